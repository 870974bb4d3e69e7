"""Policy reference counts for a batch of federated objects: the host side of kad_policyrc_count.

The policy reference counter (pkg/controllers/policyrc) keeps ``policy → number of objects referencing it`` for the
objects of one FederatedTypeConfig and writes it into each policy's ``status.typedRefCount`` and ``status.refCount``.
``reconcileCount`` (controller.go:231-278) derives, per object event, the propagation policy the object names
(``MatchedPolicyKey``) and the override policies its two labels name, and hands them to one ``Counter`` each
(counter.go:50-80): the object's previously known policies lose a reference, the new ones gain one, all of them are
flagged; ``reconcilePersist`` (controller.go:280-366) then updates a flagged policy's status where the numbers moved.

:class:`PolicyRefCounter` is the state of the reference's two Counters in one table — a policy key is
``(kind, namespace, name)`` with kind ``"propagation"`` or ``"override"`` — and turns a batch of object events into
kad_policyrc_count's arrays and its outputs back into status writes. Listing and watching objects and policies and the
``UpdateStatus`` call with its conflict retry stay with the caller.
"""

from __future__ import annotations

from typing import Dict, Hashable, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import objects as O
from .overrides import CLUSTER_OVERRIDE_POLICY_NAME_LABEL, OVERRIDE_POLICY_NAME_LABEL

PROPAGATION, OVERRIDE = "propagation", "override"
PolicyKey = Tuple[str, str, str]  # (kind, namespace, name); namespace "" for a cluster-scoped policy

# kad_policyrc_count's constants (include/kad_sched.h)
POL_EXISTS, POL_ENQUEUED = 1, 2
FLAGGED, UPDATE, NEGATIVE = 1, 2, 4

_MASK = (1 << 64) - 1


def _i64(v: int) -> int:
    """Go's int64 wrap."""
    v &= _MASK
    return v - (1 << 64) if v >> 63 else v


class PolicyRefCountError(RuntimeError):
    """The reference's panic: a policy's count fell below 0 (counter.go:69-72)."""


def referenced_policies(obj: Optional[dict], namespaced: bool) -> Tuple[PolicyKey, ...]:
    """The policies reconcileCount (controller.go:253-275) counts for one federated object; none for a deleted one.
    As in the reference, the override-policy label counts on a cluster-scoped object too, with an empty namespace
    (overrides.py does not match such a policy; the counter still counts it)."""
    if obj is None:
        return ()
    keys: List[PolicyKey] = []
    pp = O.matched_policy_key(obj, namespaced)
    if pp is not None:
        keys.append((PROPAGATION, pp[0], pp[1]))
    labels = O.get_labels(obj) or {}
    if OVERRIDE_POLICY_NAME_LABEL in labels:
        keys.append((OVERRIDE, O.get_namespace(obj), labels[OVERRIDE_POLICY_NAME_LABEL]))
    if CLUSTER_OVERRIDE_POLICY_NAME_LABEL in labels:
        keys.append((OVERRIDE, "", labels[CLUSTER_OVERRIDE_POLICY_NAME_LABEL]))
    return tuple(keys)


def _status(policy: dict) -> dict:
    s = policy.get("status")
    return s if isinstance(s, dict) else {}


class PolicyRefCounter:
    """The two Counters of the reference's controller for one type config: the known policy keys per object key,
    the key → id table and the int64 counts. A batch is ``observe`` (any number of times), ``arrays``, the call,
    ``apply``."""

    def __init__(self, type_config):
        self.ftc = type_config
        self.group, self.resource = type_config.group, type_config.plural_name  # GetTargetType().Group / .Name
        self.known: Dict[Hashable, Tuple[PolicyKey, ...]] = {}
        self.ids: Dict[PolicyKey, int] = {}
        self.keys: List[PolicyKey] = []
        self.counts: List[int] = []
        self._first: Dict[Hashable, Tuple[PolicyKey, ...]] = {}  # the batch's objects → their keys before it
        self._touched: set = set()                                # ids flagged by any event of the batch
        self._sent: Optional[dict] = None                         # the arrays of the batch in flight

    def _id(self, key: PolicyKey) -> int:
        i = self.ids.get(key)
        if i is None:
            i = self.ids[key] = len(self.keys)
            self.keys.append(key)
            self.counts.append(0)
        return i

    def observe(self, events: Iterable[Tuple[Hashable, Optional[dict]]]) -> None:
        """(qualified name, federated object or None for a deleted one) in order. Several events of one object
        collapse to first-known → last-new; the policies passed through on the way stay flagged."""
        namespaced = self.ftc.namespaced
        for name, obj in events:
            new = referenced_policies(obj, namespaced)
            prev = self.known.get(name, ())
            self._first.setdefault(name, prev)
            if new:
                self.known[name] = new
            else:
                self.known.pop(name, None)
            for key in prev + new:
                self._touched.add(self._id(key))

    def arrays(self, policies: Dict[PolicyKey, dict], enqueued: Iterable[PolicyKey] = ()) -> dict:
        """kad_policyrc_count's inputs for the events observed so far. ``policies``: the policy objects in the
        store by key; ``enqueued``: the policies a policy informer event asks to persist."""
        enq = [self._id(k) for k in enqueued]
        dec = [self.ids[k] for name, prev in self._first.items() for k in prev]
        inc = [self.ids[k] for name in self._first for k in self.known.get(name, ())]
        P = len(self.keys)
        typed, rest, total = np.zeros(P, np.int64), np.zeros(P, np.int64), np.zeros(P, np.int64)
        flags = np.zeros(P, np.uint8)
        flags[enq] |= POL_ENQUEUED
        for i, key in enumerate(self.keys):
            pol = policies.get(key)
            if pol is None:
                continue
            flags[i] |= POL_EXISTS
            st, mine, others = _status(pol), None, 0
            for t in st.get("typedRefCount") or []:
                if mine is None and t.get("group", "") == self.group and t.get("resource", "") == self.resource:
                    mine = int(t.get("count", 0))
                else:
                    others += int(t.get("count", 0))
            typed[i], rest[i], total[i] = mine or 0, _i64(others), int(st.get("refCount", 0))
        self._sent = {"dec_ids": np.array(dec, np.int32), "inc_ids": np.array(inc, np.int32),
                      "count": np.array(self.counts, np.int64), "stored_typed": typed, "stored_rest": rest,
                      "stored_total": total, "pol_flags": flags}
        return dict(self._sent)

    def apply(self, result: Optional[dict], policies: Dict[PolicyKey, dict]):
        """Stores the new counts, writes status.typedRefCount and status.refCount of the UPDATE policies in place
        (appending this (group, resource) entry as controller.go:329-335 does) and returns (the flagged keys, the
        (key, policy) pairs to UpdateStatus). ``result``: the call's outputs (None for an empty table). Raises
        PolicyRefCountError with the reference's message for the lowest policy id whose count fell below 0."""
        sent, self._sent = self._sent, None
        touched, self._touched, self._first = sorted(self._touched), set(), {}
        if sent is None or result is None or not len(sent["pol_flags"]):
            return [], []
        state = np.array(result["state"], np.uint8)
        if int(result["n_negative"][0]) or (state & NEGATIVE).any():
            ns, name = self.keys[int(np.flatnonzero(state & NEGATIVE)[0])][1:]
            raise PolicyRefCountError(f"counter.policyCounts[{{{ns} {name}}}] must be non-negative")
        new_count, new_total = result["new_count"], result["new_total"]
        # the policies an object passed through within the batch: flagged on the host, persisted by the same rule
        t = np.array(touched, np.int64)
        moved = (new_count[t] != sent["stored_typed"][t]) | (new_total[t] != sent["stored_total"][t])
        state[t] |= FLAGGED
        state[t[moved & ((sent["pol_flags"][t] & POL_EXISTS) != 0)]] |= UPDATE
        self.counts[:len(new_count)] = [int(c) for c in new_count]
        updates = []
        for i in np.flatnonzero(state & UPDATE):
            key = self.keys[i]
            pol = policies[key]
            st = pol.get("status")
            if not isinstance(st, dict):
                st = pol["status"] = {}
            typed = st.get("typedRefCount")
            if not isinstance(typed, list):
                typed = st["typedRefCount"] = []
            for entry in typed:
                if entry.get("group", "") == self.group and entry.get("resource", "") == self.resource:
                    break
            else:
                entry = {"group": self.group, "resource": self.resource} if self.group else {"resource": self.resource}
                typed.append(entry)
            entry["count"] = int(new_count[i])
            st["refCount"] = int(new_total[i])
            updates.append((key, pol))
        return [self.keys[i] for i in np.flatnonzero(state & FLAGGED)], updates

    def get_policy_counts(self, keys: Sequence[PolicyKey]) -> List[int]:
        """Counter.GetPolicyCounts (counter.go:82-92): 0 for a policy never seen."""
        return [self.counts[self.ids[k]] if k in self.ids else 0 for k in keys]
