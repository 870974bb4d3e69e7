"""Independent checker for status aggregation, object by object, written from the Go text
(pkg/controllers/statusaggregator/plugins/deployment.go:42-186, job.go:43-163). Two levels: ``run`` walks
kad_status_aggregate's columns with plain Python integers, ``deployment`` / ``job`` walk unstructured dicts. Shares
no code with kubeadmiral_amd/statusagg.py."""
import calendar
import re
import time

DEPLOYMENT, JOB = 0, 1
UPTODATE, ERROR, OLD_OTHER = 1, 2, 4
NIL, SYNCED, START, DONE, FAILED = 1, 2, 4, 8, 16
NONE_START, NONE_DONE = 2 ** 63 - 1, -2 ** 63
DEP = ("replicas", "updatedReplicas", "readyReplicas", "availableReplicas", "unavailableReplicas")
JOBF = ("active", "succeeded", "failed")


class Err(Exception):
    pass


def i32(v):
    return (v + 2 ** 31) % 2 ** 32 - 2 ** 31


# ------------------------------------------------------------------ the columns
def run(kind, obj_seg_off, obj_flags, old_vals, seg_vals, seg_flags, obj_generation=None, obj_observed=None,
        seg_observed=None, seg_synced=None, seg_start=None, seg_done=None):
    O, S = len(obj_flags), len(seg_flags)
    nv = 5 if kind == DEPLOYMENT else 3
    vals = [[int(x) for x in row] for row in seg_vals.reshape(nv, S)]
    old = [[int(x) for x in row] for row in old_vals.reshape(6 if kind == DEPLOYMENT else 5, O)]
    keys = ("sums", "changed", "observed") if kind == DEPLOYMENT else ("sums", "changed", "start_min", "done_max", "n_done", "n_failed", "finished")
    out = {k: [] for k in keys}
    out["sums"] = [[] for _ in range(nv)]
    for o in range(O):
        f = int(obj_flags[o])
        lo, hi = int(obj_seg_off[o]), int(obj_seg_off[o + 1])
        if f & ERROR:
            for k in keys:
                if k == "sums":
                    for v in range(nv):
                        out["sums"][v].append(0)
                else:
                    out[k].append(0)
            continue
        sums = [0] * nv
        differ = bool(f & OLD_OTHER)
        if kind == DEPLOYMENT:
            need = bool(f & UPTODATE)
            for s in range(lo, hi):
                sf = int(seg_flags[s])
                if sf & NIL:
                    need = False
                    continue
                if not sf & SYNCED or int(seg_synced[s]) != int(seg_observed[s]):
                    need = False
                sums = [i32(a + vals[v][s]) for v, a in enumerate(sums)]
            obs = int(obj_generation[o]) if need else int(obj_observed[o])
            out["observed"].append(obs)
            differ |= obs != old[5][o]
        else:
            start = done = None
            n_done = n_failed = 0
            for s in range(lo, hi):
                sf = int(seg_flags[s])
                if sf & NIL:
                    continue
                if sf & START and (start is None or int(seg_start[s]) < start):
                    start = int(seg_start[s])
                if sf & DONE:
                    n_done += 1
                    if done is None or done < int(seg_done[s]):
                        done = int(seg_done[s])
                elif sf & FAILED:
                    n_failed += 1
                sums = [i32(a + vals[v][s]) for v, a in enumerate(sums)]
            finished = n_done + n_failed > 0 and n_done + n_failed == hi - lo
            out["start_min"].append(NONE_START if start is None else start)
            out["done_max"].append(NONE_DONE if done is None else done)
            out["n_done"].append(n_done)
            out["n_failed"].append(n_failed)
            out["finished"].append(int(finished))
            written = done if finished and n_failed == 0 else None
            differ |= (NONE_START if start is None else start) != old[3][o]
            differ |= (NONE_DONE if written is None else written) != old[4][o]
        for v in range(nv):
            out["sums"][v].append(sums[v])
            differ |= sums[v] != old[v][o]
        out["changed"].append(int(differ))
    return out


# ------------------------------------------------------------------ unstructured objects
def go_equal(a, b):
    """reflect.DeepEqual on unstructured values."""
    if type(a) is not type(b):
        return False
    if isinstance(a, dict):
        return set(a) == set(b) and all(go_equal(a[k], b[k]) for k in a)
    if isinstance(a, list):
        return len(a) == len(b) and all(go_equal(x, y) for x, y in zip(a, b))
    return a == b


def status_of(obj):
    if "status" not in obj:
        raise Err("status not found")
    if obj["status"] is not None and not isinstance(obj["status"], dict):
        raise Err("status is not a map")
    return obj["status"]


def number(v, bits, wrap=False):
    if v is None:
        return 0
    if isinstance(v, float) and v == v and abs(v) < 1e18 and v == int(v):
        v = int(v)
    if isinstance(v, bool) or not isinstance(v, int):
        raise Err(f"{v!r} does not convert")
    if wrap:
        return i32(v)
    if not -2 ** (bits - 1) <= v < 2 ** (bits - 1):
        raise Err(f"{v!r} outside int{bits}")
    return v


def seconds(text):
    if text is None:
        return None
    m = re.fullmatch(r"(\d{4})-(\d\d)-(\d\d)T(\d\d):(\d\d):(\d\d)Z", text) if isinstance(text, str) else None
    if not m:
        raise Err(f"{text!r} is not a time this checker reads")
    return calendar.timegm(tuple(int(g) for g in m.groups()) + (0, 0, 0))


def text_of(sec):
    return time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime(sec))


def deployment(source, fed, cluster_objs, up_to_date):
    """→ (new status, status part of needUpdate); Err for the error returns."""
    need = bool(up_to_date)
    synced = {c["name"]: c.get("generation", 0) for c in ((fed or {}).get("status") or {}).get("clusters") or []}
    agg = dict.fromkeys(DEP, 0)
    for name, obj in cluster_objs.items():
        st = status_of(obj)
        if st is None:
            need = False
            continue
        member = {k: number(st.get(k), 32) for k in DEP}
        observed = number(st.get("observedGeneration"), 64)
        number(st.get("collisionCount"), 32)
        if st.get("conditions") is not None and not isinstance(st["conditions"], list):
            raise Err("conditions do not convert")
        if name not in synced or synced[name] != observed:
            need = False
        for k in DEP:
            agg[k] = i32(agg[k] + member[k])
    agg["observedGeneration"] = (source.get("metadata") or {}).get("generation", 0) if need else \
        (source.get("status") or {}).get("observedGeneration", 0)
    new = {k: float(v) for k, v in agg.items() if v}  # encoding/json decodes numbers into a map as float64
    if "status" in source and not isinstance(source["status"], dict):
        raise Err("old status is not a map")
    return new, not go_equal(new, source.get("status"))


def job(source, cluster_objs, now):
    """→ (new status, needUpdate) over the members in dict order."""
    agg = dict.fromkeys(JOBF, 0)
    start = completion = None
    completed, failed = [], []
    for name, obj in cluster_objs.items():
        st = status_of(obj)
        if st is None:
            continue
        member = {k: number(st.get(k), 32, wrap=True) for k in JOBF}
        s, c = seconds(st.get("startTime")), seconds(st.get("completionTime"))
        conds = st.get("conditions") or []
        if not isinstance(conds, list):
            raise Err("conditions do not convert")
        if start is None or (s is not None and s < start):
            start = s
        if c is not None:
            completed.append(name)
            if completion is None or completion < c:
                completion = c
        elif any(x.get("type") == "Failed" and x.get("status") == "True" for x in conds):
            failed.append(name)
        for k in JOBF:
            agg[k] = i32(agg[k] + member[k])
    new = {}
    if completed or failed:
        if len(completed) + len(failed) == len(cluster_objs):
            completed.sort()
            failed.sort()
            if completed and failed:
                t, r = "Failed", "Mixed"
                m = "Job completed in clusters [%s] and failed in member clusters [%s]" % (",".join(completed), ",".join(failed))
            elif completed:
                t, r, m = "Complete", "Completed", "Job completed in clusters [%s]" % ",".join(completed)
                new["completionTime"] = text_of(completion)
            else:
                t, r, m = "Failed", "Failed", "Job failed in clusters [%s]" % ",".join(failed)
            new["conditions"] = [{"type": t, "status": "True", "lastProbeTime": text_of(now), "lastTransitionTime": text_of(now),
                                  "reason": r, "message": m}]
    if start is not None:
        new["startTime"] = text_of(start)
    new.update({k: v for k, v in agg.items() if v})
    if "status" in source and not isinstance(source["status"], dict):
        raise Err("old status is not a map")
    return new, not go_equal(new, source.get("status"))
