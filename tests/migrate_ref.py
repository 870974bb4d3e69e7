"""Object-by-object checker for kad_migrate_estimate, in plain Python loops over the call's arrays.

Written from the Go text (pkg/controllers/automigration/util.go:29-64 countUnschedulablePods,
controller.go:292-378 estimateCapacity, :237-255 the DeepEqual of reconcile); imports nothing from
kubeadmiral_amd.automigration. Python integers do not overflow, so what this computes is the mathematical
value the int64 arithmetic of the reference yields inside the validated time domain."""

SEG_SKIP, SEG_BACKOFF = 1, 2
POD_DELETING, POD_UNSCHED, POD_TZERO = 1, 2, 4
NONE = (1 << 63) - 1


def count_unschedulable(records, now, threshold):
    """util.go:29-64 over (flags, t) records: (unschedulableCount, nextCrossIn or None)."""
    count, next_cross = 0, None
    for flags, t in records:
        if flags & POD_DELETING:                      # :35-37
            continue
        if not flags & POD_UNSCHED:                   # :47-51
            continue
        if flags & POD_TZERO:
            # the zero time: Add(threshold) stays near year 1 and Sub(now) saturates to the minimum Duration
            crossing = -(1 << 63)
        else:
            crossing = (t + threshold) - now          # :53-55
        if crossing <= 0:                             # :56-57
            count += 1
        elif next_cross is None or next_cross > crossing:  # :58-60
            next_cross = crossing
    return count, next_cross


def estimate(now, threshold, segments):
    """controller.go:292-378 for one object. segments: (cluster id, desired, flags, records) in any order.
    Returns (per segment (uns, next_cross or None, cap or None), {cluster: cap}, retry_after or None, backoff)."""
    caps, per = {}, []
    backoff, retry = False, None
    for cluster, desired, flags, records in segments:
        if flags & SEG_BACKOFF:                       # :326-328
            backoff = True
        if flags & SEG_SKIP:                          # :310-330: continue
            per.append((0, None, None))
            continue
        uns, nxt = count_unschedulable(records, now, threshold)
        if nxt is not None and (retry is None or nxt < retry):  # :341-343
            retry = nxt
        n = len(records)
        cap = n - uns if n >= desired else desired - uns  # :346-354
        if cap >= desired:                            # :356-359
            per.append((uns, nxt, None))
            continue
        if cap < 0:                                   # :360-364
            cap = 0
        caps[cluster] = cap                           # :366
        per.append((uns, nxt, cap))
    return per, caps, retry, backoff


def run(n_ids, now_ns, obj_seg_off, obj_threshold_ns, seg_cluster, seg_desired, seg_flags, seg_pod_off, pod_t_ns,
        pod_flags, old_off, old_cluster, old_cap):
    """The seven outputs of kad_migrate_estimate as lists."""
    uns, nxt, cap, changed, n_written, retry_after, backoff = [], [], [], [], [], [], []
    for o in range(len(obj_threshold_ns)):
        segs = []
        for s in range(int(obj_seg_off[o]), int(obj_seg_off[o + 1])):
            recs = [(int(pod_flags[p]), int(pod_t_ns[p])) for p in range(int(seg_pod_off[s]), int(seg_pod_off[s + 1]))]
            segs.append((int(seg_cluster[s]), int(seg_desired[s]), int(seg_flags[s]), recs))
        per, caps, retry, bo = estimate(int(now_ns), int(obj_threshold_ns[o]), segs)
        for u, x, c in per:
            uns.append(u)
            nxt.append(NONE if x is None else x)
            cap.append(-1 if c is None else c)
        existing = {int(old_cluster[q]): int(old_cap[q]) for q in range(int(old_off[o]), int(old_off[o + 1]))}
        changed.append(1 if existing != caps else 0)  # Semantic.DeepEqual: nil == empty, else keys and values
        n_written.append(len(caps))
        retry_after.append(NONE if retry is None else retry)
        backoff.append(1 if bo else 0)
    return {"uns": uns, "next_cross": nxt, "cap": cap, "changed": changed, "n_written": n_written,
            "retry_after": retry_after, "backoff": backoff}
