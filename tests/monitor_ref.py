"""An independent per-object checker of the monitor controller (pkg/controllers/monitor): meters as plain objects,
maps keyed by cluster name, and Go's time modelled exactly: a time is an integer count of nanoseconds since
0001-01-01T00:00:00Z (the zero time.Time is 0), a Duration an int64, After / Add as on integers and Sub saturating
at MinInt64 / MaxInt64 as time.Time.Sub does. Shares nothing with kubeadmiral_amd/monitor.py but the event dicts.
"""
import datetime

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
MS, SECOND, MINUTE = 10 ** 6, 10 ** 9, 60 * 10 ** 9
REPORT_INTERVAL = MINUTE
EPOCH = 62135596800 * SECOND  # 1970-01-01 in ns since year 1
_DAY0 = datetime.date(1, 1, 1).toordinal()


def go_sub(t, u):
    d = t - u
    return I64_MIN if d < I64_MIN else I64_MAX if d > I64_MAX else d


def milliseconds(d):
    return -((-d) // MS) if d < 0 else d // MS


def unix(ns):
    """A Unix-epoch time in ns as a checker time."""
    return ns + EPOCH


def parse_time(s):
    """time.Parse(time.RFC3339Nano, s) → ns since year 1, or None on error."""
    if not isinstance(s, str) or len(s) < 20 or not s.isascii():
        return None
    head, rest = s[:19], s[19:]
    if head[4] != "-" or head[7] != "-" or head[10] != "T" or head[13] != ":" or head[16] != ":":
        return None
    digits = head[:4] + head[5:7] + head[8:10] + head[11:13] + head[14:16] + head[17:19]
    if not digits.isdigit():
        return None
    y, mo, d, h, mi, sec = int(head[:4]), int(head[5:7]), int(head[8:10]), int(head[11:13]), int(head[14:16]), int(head[17:19])
    if h > 23 or mi > 59 or sec > 59:
        return None
    if y == 0:  # datetime has no year 0: proleptic Gregorian, a leap year; never used by the cases
        return None
    try:
        days = datetime.date(y, mo, d).toordinal() - _DAY0
    except ValueError:
        return None
    frac = 0
    if rest[0] in ".,":
        k = 1
        while k < len(rest) and rest[k].isdigit():
            k += 1
        if k == 1:
            return None
        frac = int(rest[1:k][:9].ljust(9, "0"))
        rest = rest[k:]
    if rest == "Z":
        off = 0
    elif len(rest) == 6 and rest[0] in "+-" and rest[3] == ":" and (rest[1:3] + rest[4:6]).isdigit():
        zh, zm = int(rest[1:3]), int(rest[4:6])
        if zh > 23 or zm > 59:
            return None
        off = (zh * 3600 + zm * 60) * (1 if rest[0] == "+" else -1)
    else:
        return None
    return (days * 86400 + h * 3600 + mi * 60 + sec - off) * SECOND + frac


class Meter:
    def __init__(self):
        self.creation = 0
        self.last_update = 0
        self.sync_success = 0
        self.last_status = None
        self.last_status_synced = 0
        self.out_of_sync = 0

    def copy(self):
        m = Meter()
        m.__dict__.update(self.__dict__)
        return m


class Panic(Exception):
    pass


class Monitor:
    """meters: the sync.Map; reconcile(event, now) → what the worker and the log line see."""

    def __init__(self):
        self.meters = {}

    def reconcile(self, ev, now):
        key, obj = ev["key"], ev.get("obj")
        out = dict(result="ALL_OK", requeue=None, update=False, last_generation=None, deleted=False, stored=False,
                   missing=False, log=None)
        if obj is None or obj.get("metadata", {}).get("deletionTimestamp") is not None:
            self.meters.pop(key, None)
            out["deleted"] = True
            return out
        meta = obj.get("metadata", {})
        if key not in self.meters:
            m = Meter()
            ct = meta.get("creationTimestamp")
            m.creation = (parse_time(ct) or 0) if ct is not None else 0  # GetCreationTimestamp: zero where it does not parse
        else:
            m = self.meters[key].copy()
        # reconcileSync
        ann = meta.get("annotations") or {}
        if "syncSuccessTimestamp" in ann:
            t = parse_time(ann["syncSuccessTimestamp"])
            if t is not None:
                m.sync_success = t
        gen = "%d" % meta.get("generation", 0)
        update = True
        if "lastGeneration" in ann:
            if gen != ann["lastGeneration"]:
                m.last_update = now
                if "lastSyncSuccessGeneration" in ann and gen == ann["lastSyncSuccessGeneration"]:
                    m.last_update = m.sync_success - 10 * MS
            else:
                if "lastSyncSuccessGeneration" in ann and gen == ann["lastSyncSuccessGeneration"]:
                    if m.last_update > m.sync_success:
                        m.last_update = m.sync_success - 10 * MS
                update = False
        out["update"] = update
        out["last_generation"] = gen if update else None
        self.meters[key] = m.copy()
        if ev.get("status_enabled"):
            st = ev.get("status")
            if st is None or st.get("metadata", {}).get("deletionTimestamp") is not None:
                return out
            err = self._status(ev, m, now)
            out["log"] = (None if m.last_status is None else dict(m.last_status), m.last_status_synced, m.out_of_sync)
            if err == "out-of-sync":
                out["result"], out["requeue"] = "REQUEUE", 5
                return out
            if err == "missing":
                out["missing"] = True
                return out
            if err is not None:
                out["result"] = "ERROR"
                return out
            self.meters[key] = m
            out["stored"] = True
        return out

    @staticmethod
    def _status(ev, m, now):
        fed = {}
        entries = ev["status"].get("clusterStatus")
        for e in entries if isinstance(entries, list) else []:
            if e is None or e.get("clusterName") is None:
                return "missing"
            name = e["clusterName"]
            if not isinstance(name, str):
                raise Panic("clusterName")
            if e.get("status") is not None and not isinstance(e["status"], dict):
                raise Panic("status")
            if e.get("status") is None or e["status"].get("observedGeneration") is None:
                return "missing"
            g = e["status"]["observedGeneration"]
            if isinstance(g, bool) or not isinstance(g, int):
                raise Panic("observedGeneration")
            fed[name] = g
        cluster = {}
        for name, o in ev.get("members") or []:
            g = (o.get("status") or {}).get("observedGeneration") if isinstance(o.get("status"), dict) else None
            if isinstance(g, bool) or not isinstance(g, int):
                return "cluster"
            cluster[name] = g
        if m.last_status is None:
            m.last_status = cluster
            m.last_status_synced = now
            return None
        if cluster == fed:
            m.out_of_sync = 0
            m.last_status_synced = now
            m.last_status = cluster
            return None
        if m.last_status == cluster:
            m.out_of_sync = go_sub(now, m.last_status_synced)
        else:
            if m.out_of_sync == 0:
                m.out_of_sync = SECOND
                m.last_status_synced = now
            else:
                m.out_of_sync = go_sub(now, m.last_status_synced)
            m.last_status = cluster
        return "out-of-sync"

    def report(self, now):
        """DoReport → {counts by metric name, type_sync / type_status by kind (non-zero only), sync / status timers
        by meter key, the two throughputs}."""
        names = (("latency5min", 5), ("latency10min", 10), ("latency30min", 30), ("latency1hour", 60),
                 ("latency6hour", 180), ("latency1day", 1440))
        lat = {n: [mins, 0, 0] for n, mins in names}
        type_sync, type_status = {}, {}
        for k, m in self.meters.items():
            start = m.creation
            if m.last_update > m.creation:
                start = m.last_update
            if start > m.sync_success:
                for mk, mv in lat.items():
                    kind = k.split("/")[0]
                    if now > start + mv[0] * MINUTE:
                        mv[1] += 1
                        if mk == "latency5min":
                            type_sync[kind] = type_sync.get(kind, 0) + 1
                    if m.out_of_sync > mv[0] * MINUTE:
                        mv[2] += 1
                        if mk == "latency5min":
                            type_status[kind] = type_status.get(kind, 0) + 1
        counts = {}
        for k, v in lat.items():
            counts[k + ".count"] = v[1]
            counts[k + ".status.count"] = v[2]
        sync_timers, status_timers = {}, {}
        for k, m in self.meters.items():
            if m.sync_success + REPORT_INTERVAL > now:
                start = m.creation
                if m.last_update > m.creation:
                    start = m.last_update
                if m.sync_success > start:
                    sync_timers[k] = milliseconds(go_sub(m.sync_success, start))
        for k, m in self.meters.items():
            if m.last_status_synced == 0:
                continue
            if m.out_of_sync > REPORT_INTERVAL:
                status_timers[k] = milliseconds(m.out_of_sync)
        return dict(counts=counts, type_sync=type_sync, type_status=type_status, sync_timers=sync_timers,
                    status_timers=status_timers, sync_throughput=len(sync_timers), status_throughput=len(status_timers))

    def metrics(self, now):
        """The report as a sorted list of (op, name, value, tags): the reference's order is unspecified."""
        r = self.report(now)
        m = [("store", k, v, ()) for k, v in r["counts"].items()]
        m += [("store", "typelatency5min.count", v, (("type", k),)) for k, v in r["type_sync"].items()]
        m += [("store", "typelatency5min.status.count", v, (("type", k),)) for k, v in r["type_status"].items()]
        m += [("timer", "totalsync.latency.ms", v, (("resourcename", k),)) for k, v in r["sync_timers"].items()]
        m += [("timer", "totalstatus.latency.ms", v, (("resourcename", k),)) for k, v in r["status_timers"].items()]
        m += [("store", "totalsync.throughput", r["sync_throughput"], ()),
              ("store", "totalstatus.throughput", r["status_throughput"], ())]
        return sorted(m)
