"""Two checkers of the policy reference counts that share no code with the product.

``Counter`` and ``Controller`` restate pkg/controllers/policyrc one event at a time over dicts: Counter.Update
(counter.go:50-80), reconcileCount (controller.go:231-278) and reconcilePersist (controller.go:280-366). ``run`` is
kad_policyrc_count's array-level answer in numpy (np.add.at over the two id lists)."""
import numpy as np

POL_EXISTS, POL_ENQUEUED = 1, 2
FLAGGED, UPDATE, NEGATIVE = 1, 2, 4

PP_LABEL = "kubeadmiral.io/propagation-policy-name"
CPP_LABEL = "kubeadmiral.io/cluster-propagation-policy-name"
OP_LABEL = "kubeadmiral.io/override-policy-name"
COP_LABEL = "kubeadmiral.io/cluster-override-policy-name"


def wrap(v):
    """Go's int64 arithmetic."""
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >= 1 << 63 else v


class Counter:
    """counter.go: knownPolicies, policyCounts and the keys handed to flagPolicyNeedUpdate, in order."""

    def __init__(self):
        self.known, self.counts, self.flagged = {}, {}, []

    def update(self, obj, new_policies):
        previous = self.known.get(obj, [])
        if len(new_policies) > 0:
            self.known[obj] = list(new_policies)
        else:
            self.known.pop(obj, None)
        for p in previous:
            self.counts[p] = self.counts.get(p, 0) - 1
            if self.counts[p] < 0:
                raise RuntimeError("counter.policyCounts[{%s %s}] must be non-negative" % p)
            self.flagged.append(p)
        for p in new_policies:
            self.counts[p] = self.counts.get(p, 0) + 1
        self.flagged.extend(new_policies)

    def get_policy_counts(self, keys):
        return [self.counts.get(k, 0) for k in keys]


class Controller:
    """The controller around its two Counters for one type config; policy keys are (namespace, name)."""

    def __init__(self, group, resource, namespaced):
        self.group, self.resource, self.namespaced = group, resource, namespaced
        self.pp, self.op = Counter(), Counter()

    def reconcile_count(self, name, obj):
        """controller.go:253-275; obj None: the store no longer holds it."""
        new_pps, new_ops = [], []
        if obj is not None:
            meta = obj.get("metadata", {})
            labels, ns = meta.get("labels") or {}, meta.get("namespace", "")
            if PP_LABEL in labels and self.namespaced:  # MatchedPolicyKey, scheduler/util.go:37-49
                new_pps = [(ns, labels[PP_LABEL])]
            elif CPP_LABEL in labels:
                new_pps = [("", labels[CPP_LABEL])]
            if OP_LABEL in labels:
                new_ops.append((ns, labels[OP_LABEL]))
            if COP_LABEL in labels:
                new_ops.append(("", labels[COP_LABEL]))
        self.pp.update(name, new_pps)
        self.op.update(name, new_ops)

    def reconcile_persist(self, counter, key, policy):
        """controller.go:307-353 on the stored policy (None: not in the store): writes it, returns hasChange."""
        if policy is None:
            return False
        status = policy.setdefault("status", {})
        typed = status.setdefault("typedRefCount", [])
        matched = None
        for t in typed:
            if t.get("group", "") == self.group and t.get("resource", "") == self.resource:
                matched = t
                break
        if matched is None:
            matched = {"resource": self.resource, "count": 0}
            if self.group:
                matched["group"] = self.group
            typed.append(matched)
        new = counter.get_policy_counts([key])[0]
        change = False
        if new != matched.get("count", 0):
            matched["count"] = new
            change = True
        total = 0
        for t in typed:
            total = wrap(total + t.get("count", 0))
        if total != status.get("refCount", 0):
            status["refCount"] = total
            change = True
        return change


def run(dec_ids, inc_ids, count, stored_typed, stored_rest, stored_total, pol_flags, **_):
    """kad_policyrc_count's outputs."""
    count = np.asarray(count, np.int64)
    P = len(count)
    dec, inc = np.zeros(P, np.int64), np.zeros(P, np.int64)
    np.add.at(dec, np.asarray(dec_ids, np.int64), 1)
    np.add.at(inc, np.asarray(inc_ids, np.int64), 1)
    with np.errstate(over="ignore"):
        new_count = count + inc - dec
        new_total = np.asarray(stored_rest, np.int64) + new_count
    pf = np.asarray(pol_flags, np.uint8)
    flagged = (dec > 0) | (inc > 0)
    update = ((pf & POL_EXISTS) != 0) & (flagged | ((pf & POL_ENQUEUED) != 0)) & \
        ((new_count != np.asarray(stored_typed, np.int64)) | (new_total != np.asarray(stored_total, np.int64)))
    negative = new_count < 0
    state = (flagged * FLAGGED + update * UPDATE + negative * NEGATIVE).astype(np.uint8)
    return {"new_count": new_count, "new_total": new_total, "state": state,
            "n_negative": np.array([int(negative.sum())], np.int32)}
