"""Shapes for kad_migrate_estimate: batches as the call's arrays, built object by object.

The existing annotation of an object is derived from the checker's own result for it (migrate_ref.estimate) —
equal, lacking its last entry, with its last value altered, with one more key, or empty — so every DeepEqual
branch occurs at every object size."""
import numpy as np

import migrate_ref as R

SEC = 10**9
NOW = 1_760_000_000 * SEC
TMAX = 1 << 61
N_IDS = 130
OLD_KINDS = ("same", "drop_last", "alter_last", "extra", "empty")


class Builder:
    def __init__(self, n_ids=N_IDS, now=NOW):
        self.n_ids, self.now = n_ids, now
        self.so, self.thr = [0], []
        self.sc, self.sd, self.sf, self.po = [], [], [], [0]
        self.pt, self.pf = [], []
        self.oo, self.oc, self.ov = [0], [], []

    def add(self, threshold, segments, old="same"):
        """segments: (cluster, desired, flags, [(pod flags, t), ...]) with ascending clusters; old: one of
        OLD_KINDS or an explicit {cluster: cap}."""
        for c, d, f, recs in segments:
            self.sc.append(c)
            self.sd.append(d)
            self.sf.append(f)
            self.pf += [r[0] for r in recs]
            self.pt += [r[1] for r in recs]
            self.po.append(len(self.pt))
        self.so.append(len(self.sc))
        self.thr.append(threshold)
        if not isinstance(old, dict):
            caps = dict(R.estimate(self.now, threshold, segments)[1])
            keys = sorted(caps)
            if old == "drop_last" and keys:
                del caps[keys[-1]]
            elif old == "alter_last" and keys:
                caps[keys[-1]] += 1
            elif old == "extra":
                caps[next(i for i in range(self.n_ids - 1, -1, -1) if i not in caps)] = 3
            elif old == "empty":
                caps = {}
            old = caps
        for c in sorted(old):
            self.oc.append(c)
            self.ov.append(old[c])
        self.oo.append(len(self.oc))
        return len(self.thr) - 1

    def arrays(self):
        return dict(n_ids=self.n_ids, now_ns=self.now, obj_seg_off=np.array(self.so, np.int32),
                    obj_threshold_ns=np.array(self.thr, np.int64), seg_cluster=np.array(self.sc, np.int32),
                    seg_desired=np.array(self.sd, np.int64), seg_flags=np.array(self.sf, np.uint8),
                    seg_pod_off=np.array(self.po, np.int64), pod_t_ns=np.array(self.pt, np.int64),
                    pod_flags=np.array(self.pf, np.uint8), old_off=np.array(self.oo, np.int32),
                    old_cluster=np.array(self.oc, np.int32), old_cap=np.array(self.ov, np.int64))


def pods(rng, n, now, threshold, unsched=0.5):
    """n pod records around the crossing instant: about half of the unschedulable ones have crossed, a few
    cross exactly now (counted) or one nanosecond from now (not counted: the minimum), a few are deleting or
    lack a transition time."""
    out = []
    cut = now - threshold
    for _ in range(n):
        f = R.POD_UNSCHED if rng.random() < unsched else 0
        if rng.random() < 0.1:
            f |= R.POD_DELETING
        t = cut + int(rng.integers(-90 * SEC, 90 * SEC))
        x = rng.random()
        if x < 0.03:
            t = cut
        elif x < 0.06:
            t = cut + 1
        elif x < 0.08 and f & R.POD_UNSCHED:
            f |= R.POD_TZERO
            t = 0
        out.append((f, t))
    return out


def lengths(long_min):
    return [0, 1, 7, 8, 9, 63, 64, 65, long_min - 1, long_min, long_min + 1, 3 * 256 + 5]


def shapes_case(long_min, seed=5, pad_segments=0):
    """Every segment length at which a path changes, each as its own object under every OLD_KINDS; objects with
    0, 1, 2 and 65 segments; skipped segments between live ones; a backoff-only object; an object whose
    segments alternate long and empty. ``pad_segments`` more one-pod segments (in objects of four) lower the
    batch's mean segment length, and with it the route's group width."""
    rng = np.random.default_rng(seed)
    b = Builder()
    thr = 60 * SEC
    for k, n in enumerate(lengths(long_min)):
        for j, old in enumerate(OLD_KINDS if n in (0, 9, long_min + 1) else ("same", "alter_last")):
            desired = n + (3, 0, -1)[(k + j) % 3]  # n < desired, n == desired, n > desired
            b.add(thr, [((k * 7 + j) % N_IDS, max(desired, 1), 0, pods(rng, n, NOW, thr))], old)
    marks = {}
    marks["no-segments"] = b.add(thr, [], "same")
    marks["no-segments-stale"] = b.add(thr, [], {4: 1})
    for nseg in (1, 2, 65):
        for old in OLD_KINDS:
            segs = [(c * 2, int(rng.integers(1, 12)), 0, pods(rng, int(rng.integers(0, 10)), NOW, thr, 0.8)) for c in range(nseg)]
            marks[f"{nseg}-segments-{old}"] = b.add(thr, segs, old)
    # skipped segments between live ones: their pods, if any, are not read and they feed nothing
    segs = []
    for c in range(12):
        f = (0, R.SEG_SKIP, R.SEG_SKIP | R.SEG_BACKOFF)[c % 3]
        segs.append((c, 9, f, pods(rng, 6, NOW, thr, 0.9)))
    marks["interleaved"] = b.add(thr, segs, "same")
    marks["backoff-only"] = b.add(thr, [(3, 5, R.SEG_SKIP | R.SEG_BACKOFF, []), (9, 5, R.SEG_SKIP, [])], {3: 2})
    marks["skip-only"] = b.add(thr, [(3, 5, R.SEG_SKIP, pods(rng, 4, NOW, thr, 1.0))], "same")
    # all pods deleting: they count in len(pods) and nowhere else
    dele = [(R.POD_DELETING | R.POD_UNSCHED, NOW - 2 * thr)] * 5
    marks["all-deleting"] = b.add(thr, [(1, 5, 0, dele), (2, 9, 0, dele)], "same")
    # a negative threshold: pods that became unschedulable up to |threshold| in the future have crossed
    marks["negative-threshold"] = b.add(-30 * SEC, [(7, 4, 0, [(R.POD_UNSCHED, NOW + 30 * SEC), (R.POD_UNSCHED, NOW + 30 * SEC + 1),
                                                               (R.POD_UNSCHED, NOW + 31 * SEC), (R.POD_UNSCHED, NOW)])], "empty")
    # crossing exactly 0 counts; + 1 ns does not and is the minimum
    marks["exact"] = b.add(thr, [(8, 3, 0, [(R.POD_UNSCHED, NOW - thr), (R.POD_UNSCHED, NOW - thr + 1),
                                            (R.POD_UNSCHED, NOW - thr + 5)])], "empty")
    marks["desired-0"] = b.add(thr, [(8, 0, 0, pods(rng, 3, NOW, thr, 1.0)), (9, -4, 0, pods(rng, 3, NOW, thr, 1.0))], "same")
    segs = [(c, long_min + 40, 0, pods(rng, (long_min + 9) if c % 2 == 0 else 0, NOW, thr)) for c in range(8)]
    marks["long-empty-alternating"] = b.add(thr, segs, "alter_last")
    for k in range(0, pad_segments, 4):
        b.add(thr, [(c, 2, 0, pods(rng, 1, NOW, thr, 0.7)) for c in range(min(4, pad_segments - k))], "same")
    return b.arrays(), marks


def object_width_case(nseg, seed=8):
    """Five objects of ``nseg`` short segments, one under each of OLD_KINDS, then one of a single segment and one
    of none: the mean number of segments per object decides the object kernel's group width."""
    rng = np.random.default_rng(seed)
    b = Builder()
    thr = 60 * SEC
    for old in OLD_KINDS:
        b.add(thr, [(c * 2, int(rng.integers(1, 12)), (0, 0, R.SEG_SKIP)[c % 3], pods(rng, int(rng.integers(0, 10)), NOW, thr, 0.8))
                    for c in range(nseg)], old)
    b.add(thr, [(5, 4, 0, pods(rng, 4, NOW, thr, 1.0))], "drop_last")
    b.add(thr, [], "same")
    return b.arrays()


def edge_case(now):
    """t, threshold and now at the edges of the time domain (|.| <= 2^61, 0 <= now)."""
    b = Builder(now=now)
    U = R.POD_UNSCHED
    b.add(TMAX, [(0, 4, 0, [(U, TMAX), (U, -TMAX), (U, 0), (U, now)])], "empty")
    b.add(-TMAX, [(0, 4, 0, [(U, TMAX), (U, -TMAX), (U, 0), (U | R.POD_TZERO, 12345)])], "empty")
    b.add(0, [(5, 9, 0, [(U, now), (U, min(now + 1, TMAX)), (U, TMAX), (U, -TMAX)]), (6, 2, 0, [(U, now - 1 if now else 0)])], "same")
    return b.arrays()


def as_lists(r):
    return {k: [int(x) for x in v] for k, v in r.items()}
