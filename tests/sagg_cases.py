"""Shapes for kad_status_aggregate's tests: batches as the call's arrays, built directly (no objects), so that
values the object formats cannot carry (times at the edge of the domain) are reachable."""
import numpy as np

import sagg_ref as R

WIDTHS = (1, 2, 4, 8, 16, 32, 64)
TMAX = 1 << 61


def lengths(long_min):
    """Segments per object: 0, 1, W - 1 / W / W + 1 for every group width, 63 / 64 / 65, long_min - 1 / + 0 / + 1 and
    3 * 256 + 5."""
    s = {0, 1, 3 * 256 + 5, long_min - 1, long_min, long_min + 1}
    for w in WIDTHS:
        s |= {w - 1, w, w + 1}
    return sorted(s)


def batch(kind, lens, seed=0, stale_every=3):
    """A batch with ``lens[i]`` random segments for object i; the old status of every ``stale_every``-th object
    differs from the new one, the others hold exactly the new one (from the checker)."""
    rng = np.random.default_rng([seed, kind, 0x5A66])
    O, S = len(lens), int(sum(lens))
    nv = 5 if kind == R.DEPLOYMENT else 3
    off = np.zeros(O + 1, np.int32)
    off[1:] = np.cumsum(lens)
    a = dict(kind=kind, obj_seg_off=off, obj_flags=(rng.random(O) < 0.7).astype(np.uint8) * R.UPTODATE,
             old_vals=np.zeros((6 if kind == R.DEPLOYMENT else 5, O), np.int64),
             seg_vals=rng.integers(0, 50, (nv, S)).astype(np.int32))
    nil = rng.random(S) < 0.05
    if kind == R.DEPLOYMENT:
        gen = rng.integers(1, 9, S)
        a.update(obj_generation=rng.integers(1, 100, O).astype(np.int64), obj_observed=rng.integers(0, 100, O).astype(np.int64),
                 seg_observed=gen.astype(np.int64), seg_synced=np.where(rng.random(S) < 0.1, gen - 1, gen).astype(np.int64),
                 seg_flags=np.where(nil, R.NIL, np.where(rng.random(S) < 0.95, R.SYNCED, 0)).astype(np.uint8))
    else:
        start = rng.integers(1_600_000_000, 1_700_000_000, S)
        has_start, cls = rng.random(S) < 0.9, rng.random(S)
        f = np.where(has_start, R.START, 0) | np.where(cls < 0.6, R.DONE, np.where(cls < 0.8, R.FAILED, 0))
        a.update(seg_start=start.astype(np.int64), seg_done=(start + rng.integers(0, 5000, S)).astype(np.int64),
                 seg_flags=np.where(nil, R.NIL, f).astype(np.uint8))
        a["old_vals"][3], a["old_vals"][4] = R.NONE_START, R.NONE_DONE
    return settle(a, stale_every)


def settle(a, stale_every=3):
    """Give the objects their own new status as the old one, except every ``stale_every``-th."""
    r = R.run(**a)
    kind, O = a["kind"], len(a["obj_flags"])
    nv = 5 if kind == R.DEPLOYMENT else 3
    for o in range(O):
        if stale_every and o % stale_every == stale_every - 1:
            continue
        for v in range(nv):
            a["old_vals"][v, o] = r["sums"][v][o]
        if kind == R.DEPLOYMENT:
            a["old_vals"][5, o] = r["observed"][o]
        else:
            a["old_vals"][3, o] = r["start_min"][o]
            a["old_vals"][4, o] = r["done_max"][o] if r["finished"][o] and not r["n_failed"][o] else R.NONE_DONE
    return a


def shapes_case(kind, long_min, seed=0):
    """The lengths of :func:`lengths` (each twice) with the named edge objects between them; → (arrays, marks)."""
    items = [(None, n) for n in lengths(long_min) for _ in range(2)]
    for j, item in enumerate((("error", 5), ("all-nil", 4), ("wrap", 3), ("edge-times", 4), ("error-long", long_min + 3))):
        items.insert(3 + 4 * j, item)  # between live objects
    marks = {name: i for i, (name, _) in enumerate(items) if name}
    a = batch(kind, [n for _, n in items], seed)
    off = a["obj_seg_off"]

    def segs(name):
        return slice(int(off[marks[name]]), int(off[marks[name] + 1]))

    a["obj_flags"][marks["error"]] |= R.ERROR
    a["obj_flags"][marks["error-long"]] |= R.ERROR
    a["seg_flags"][segs("all-nil")] = R.NIL
    a["seg_vals"][:, segs("wrap")] = np.array([[2 ** 31 - 1, 1, 5], [-2 ** 31, -1, -7], [2 ** 30, 2 ** 30, 2 ** 30]] +
                                              [[7, 8, 9]] * (2 if kind == R.DEPLOYMENT else 0), np.int32)
    if kind == R.DEPLOYMENT:
        a["seg_flags"][segs("wrap")] = R.SYNCED
        a["seg_observed"][segs("edge-times")] = [2 ** 63 - 1, -2 ** 63, 0, 5]
        a["seg_synced"][segs("edge-times")] = [2 ** 63 - 1, -2 ** 63, 0, 5]
        a["seg_flags"][segs("edge-times")] = R.SYNCED
        a["obj_flags"][marks["edge-times"]] |= R.UPTODATE
    else:
        a["seg_flags"][segs("wrap")] = R.START | R.DONE
        a["seg_flags"][segs("edge-times")] = R.START | R.DONE
        a["seg_start"][segs("edge-times")] = [TMAX, -TMAX, 0, TMAX - 1]
        a["seg_done"][segs("edge-times")] = [-TMAX, TMAX, 1, -TMAX + 1]
    a["old_vals"][:] = 0
    if kind == R.JOB:
        a["old_vals"][3], a["old_vals"][4] = R.NONE_START, R.NONE_DONE
    return settle(a), marks
