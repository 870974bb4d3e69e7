"""Override policies: which override rules apply to which placed cluster, for a batch of objects.

The override-policy controller runs after the scheduler on every federated
object (``pkg/controllers/override/overridepolicy_controller.go:254-376``):
it looks up the object's ClusterOverridePolicy and OverridePolicy
(``lookForMatchedPolicies``, ``override/util.go:45-97``), asks for every placed
cluster and every override rule whether the rule's target clusters select the
cluster (``parseOverrides`` / ``isClusterMatched``, ``util.go:99-221``), merges
the patches of the matching rules per cluster (``mergeOverrides``,
``util.go:142-152``) and writes them into the object under its own controller
name. The (rule, cluster) evaluation is the device's part
(``kad_override_match``, ``include/kad_sched.h``); this module holds the
types (``pkg/apis/core/v1alpha1/types_overridepolicy.go``), the policy lookup,
the packer of a policy set (:class:`PolicySet`) and the assembly of the
device's rule bits into overrides maps.
"""

from __future__ import annotations

import ctypes
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import gojson as J
from . import k8s
from . import objects as O
from . import types as T
from .pack import (ABI_VERSION, TERM_EXPR_VALID, TERM_FIELD_VALID, TERM_HAS_EXPR, TERM_HAS_FIELD, Snapshot, _assemble,
                   _Compiler, _csr, _valid_requirement)

# overridepolicy_controller.go:48-57
CONTROLLER_NAME = "overridepolicy-controller"
PREFIXED_CONTROLLER_NAME = O.DEFAULT_PREFIX + CONTROLLER_NAME
OVERRIDE_POLICY_NAME_LABEL = O.DEFAULT_PREFIX + "override-policy-name"
CLUSTER_OVERRIDE_POLICY_NAME_LABEL = O.DEFAULT_PREFIX + "cluster-override-policy-name"

OVERRIDE_MAGIC = 0x4F44414B  # "KADO"
(O_POL_RULE_OFF, O_RULE_FLAGS, O_RULE_NAME_OFF, O_RULE_NAME, O_RULE_PROG_OFF, O_RULE_PROG, O_REQ_OFF, O_REQ,
 O_NARRAYS) = range(9)
OVR_HAS_TARGET, OVR_HAS_NAMES, OVR_SEL_INVALID, OVR_BAD_VALUE = 1, 2, 4, 8

OverridePatch = O._OverridePatch  # types/v1alpha1 OverridePatch: op, path, value
OverridesMap = Dict[str, List[OverridePatch]]  # util.OverridesMap: cluster name → patches


# ------------------------------------------------------------------- types
@dataclass
class JsonPatchOverrider:  # types_overridepolicy.go JsonPatchOverrider
    operator: str = ""
    path: str = ""
    value: bytes = b""  # apiextensionsv1.JSON.Raw


@dataclass
class TargetClusters:  # types_overridepolicy.go TargetClusters
    clusters: Optional[List[str]] = None
    cluster_selector: Optional[Dict[str, str]] = None
    cluster_affinity: Optional[List[T.ClusterSelectorTerm]] = None


@dataclass
class OverrideRule:  # types_overridepolicy.go OverrideRule (Overriders.JsonPatch flattened)
    target_clusters: Optional[TargetClusters] = None
    json_patch: List[JsonPatchOverrider] = field(default_factory=list)


@dataclass
class OverridePolicy:
    """An OverridePolicy (``namespace`` set) or a ClusterOverridePolicy (``namespace`` None)."""
    name: str = ""
    namespace: Optional[str] = None
    rules: List[OverrideRule] = field(default_factory=list)

    def key(self) -> str:
        return self.name if not self.namespace else self.namespace + "/" + self.name

    def kind(self) -> str:
        return "OverridePolicy" if self.namespace else "ClusterOverridePolicy"


class OverrideError(Exception):
    """An error of the reference's reconcile for one object: ``reason`` is its event reason
    (``MatchOverridePolicyFailed`` from the lookup, ``ParseOverridePolicyFailed`` from parseOverrides)."""

    def __init__(self, reason: str, policy: Optional[str], msg: str, recheck: bool = False):
        super().__init__(msg)
        self.reason, self.policy, self.recheck = reason, policy, recheck

    def __eq__(self, other):
        return isinstance(other, OverrideError) and (self.reason, self.policy) == (other.reason, other.policy)

    __hash__ = Exception.__hash__


MATCH_FAILED, PARSE_FAILED = "MatchOverridePolicyFailed", "ParseOverridePolicyFailed"


# ---------------------------------------------------------- lookup and merge
def look_for_matched_policies(obj, is_namespaced: bool, policies: Dict[str, OverridePolicy],
                              cluster_policies: Dict[str, OverridePolicy]
                              ) -> Tuple[Optional[List[OverridePolicy]], bool, Optional[str]]:
    """lookForMatchedPolicies (override/util.go:45-97) over two stores keyed as the informer caches are
    (``name`` / ``namespace/name``) → (policies, needs recheck on error, error message or None). A dict
    lookup cannot fail, so the recheck flag (set only on store errors, :62-64, :83-85) is always False."""
    found: List[OverridePolicy] = []
    labels = O.get_labels(obj) or {}
    if CLUSTER_OVERRIDE_POLICY_NAME_LABEL in labels:
        name = labels[CLUSTER_OVERRIDE_POLICY_NAME_LABEL]
        if len(name) == 0:
            return None, False, "policy name cannot be empty"
        pol = cluster_policies.get(name)
        if pol is None:
            return None, False, f"ClusterOverridePolicy {name} not found"
        found.append(pol)
    if is_namespaced and OVERRIDE_POLICY_NAME_LABEL in labels:
        name = labels[OVERRIDE_POLICY_NAME_LABEL]
        if len(name) == 0:
            return None, False, "policy name cannot be empty"
        key = O.get_namespace(obj) + "/" + name
        pol = policies.get(key)
        if pol is None:
            return None, False, f"OverridePolicy {key} not found"
        found.append(pol)
    return found, False, None


def merge_overrides(dest: Optional[OverridesMap], src: OverridesMap) -> OverridesMap:
    """mergeOverrides (override/util.go:142-152)."""
    if dest is None:
        dest = {}
    for cluster, patches in src.items():
        dest[cluster] = list(dest.get(cluster) or []) + list(patches)
    return dest


def decode_value(raw: bytes):
    """policyJsonPatchOverriderToOverridePatch's value (util.go:231-237): an empty raw value is not
    decoded (nil); raises :class:`gojson.GoJSONError` when json.Unmarshal would fail."""
    if len(raw) == 0:
        return None
    return J.unmarshal(bytes(raw).decode("utf-8", "replace"), J.ANY)


def _value_decodes(raw: bytes) -> bool:
    try:
        decode_value(raw)
        return True
    except J.GoJSONError:
        return False


def selector_valid(sel: Optional[Dict[str, str]]) -> bool:
    """metav1.LabelSelectorAsSelector{MatchLabels}: every pair through NewRequirement(k, In, [v])."""
    return all(k8s.is_qualified_name(k) and k8s.is_valid_label_value(v) for k, v in (sel or {}).items())


# ------------------------------------------------------------------ packer
class OverrideHeader(ctypes.Structure):  # kad_override_header
    _fields_ = [("magic", ctypes.c_uint32), ("abi_version", ctypes.c_uint32), ("n_policies", ctypes.c_int32),
                ("n_rules", ctypes.c_int32), ("n_reqs", ctypes.c_int32), ("n_clusters", ctypes.c_int32),
                ("total_bytes", ctypes.c_uint64), ("snapshot_fingerprint", ctypes.c_uint64),
                ("off", ctypes.c_uint64 * O_NARRAYS)]


class PolicySet:
    """A packed set of (Cluster)OverridePolicies against one Snapshot (``kad_override_header`` blob).

    Policy p's rules are ``[pol_rule_off[p], pol_rule_off[p + 1])``; requirements are interned set-wide
    and encoded as ``KAD_B_REQ``; a rule's target program has the ClusterAffinity filter-program format.
    """

    def __init__(self, snap: Snapshot, policies: Sequence[OverridePolicy]):
        self.snap = snap
        self.policies = list(policies)
        self.index = {id(p): i for i, p in enumerate(self.policies)}
        comp = _Compiler(snap)
        pol_off = [0]
        flags: List[int] = []
        names: List[list] = []
        progs: List[list] = []
        self.rules: List[OverrideRule] = []
        for pol in self.policies:
            for rule in pol.rules:
                f, nm, prog = self._rule(comp, rule)
                flags.append(f)
                names.append(nm)
                progs.append(prog)
                self.rules.append(rule)
            pol_off.append(len(flags))
        name_off, name_a = _csr(names, np.int32)
        prog_off, prog_a = _csr(progs, np.int32)
        req_off, req_a = _csr(comp.reqs, np.int32)
        self.pol_rule_off = np.array(pol_off, np.int32)
        arrays = [self.pol_rule_off, np.array(flags, np.uint32), name_off, name_a, prog_off, prog_a, req_off, req_a]
        hdr = OverrideHeader()
        hdr.magic, hdr.abi_version = OVERRIDE_MAGIC, ABI_VERSION
        hdr.n_policies, hdr.n_rules, hdr.n_reqs, hdr.n_clusters = len(self.policies), len(flags), len(comp.reqs), snap.C
        hdr.snapshot_fingerprint = snap.fingerprint
        self.blob = _assemble(hdr, arrays)
        self.arrays = arrays
        self.P, self.R = len(self.policies), len(flags)

    @staticmethod
    def _rule(comp: _Compiler, rule: OverrideRule):
        f = 0
        if any(not _value_decodes(o.value) for o in rule.json_patch or []):
            f |= OVR_BAD_VALUE
        tc = rule.target_clusters
        if tc is None:
            return f, [], [0, 0]
        f |= OVR_HAS_TARGET
        ids: List[int] = []
        if len(tc.clusters or []) > 0:
            f |= OVR_HAS_NAMES
            ids = sorted({comp.snap.name_id[n] for n in tc.clusters if n in comp.snap.name_id})
        if not selector_valid(tc.cluster_selector):
            return f | OVR_SEL_INVALID, ids, [0, 0]
        sel = tc.cluster_selector or {}
        prog = [len(sel)] + [comp.intern(comp.eq_req(k, v)) for k, v in sel.items()]
        terms = tc.cluster_affinity or []
        if len(terms) == 0:
            return f, ids, prog + [0]
        prog += [1, len(terms)]
        for t in terms:
            exprs, fields = t.match_expressions or [], t.match_fields or []
            tf, body_e, body_f = 0, [], []
            if exprs:
                tf |= TERM_HAS_EXPR
                if all(_valid_requirement(r) for r in exprs):
                    tf |= TERM_EXPR_VALID
                    body_e = [comp.intern(comp.label_req(r)) for r in exprs]
            if fields:
                tf |= TERM_HAS_FIELD
                if comp._valid_fields(fields):
                    tf |= TERM_FIELD_VALID
                    body_f = [comp.intern(comp.field_req(r)) for r in fields]
            prog += [tf, len(body_e), len(body_f)] + body_e + body_f
        return f, ids, prog

    def policy_index(self, pol: Optional[OverridePolicy]) -> int:
        return -1 if pol is None else self.index[id(pol)]

    def rule_words(self, obj_policy: np.ndarray) -> int:
        """The smallest RW (u32 words per slot row) that holds every listed object's rule list."""
        n = np.diff(self.pol_rule_off)
        op = np.asarray(obj_policy, np.int64).reshape(-1, 2)
        cnt = np.where(op >= 0, n[np.clip(op, 0, max(0, self.P - 1))] if self.P else 0, 0).sum(axis=1)
        return max(1, (int(cnt.max()) + 31) // 32) if len(cnt) else 1


# ---------------------------------------------------------------- assembly
def _patches(rule: OverrideRule) -> List[OverridePatch]:
    return [OverridePatch(o.operator, o.path, decode_value(o.value)) for o in rule.json_patch or []]


def assemble(pset: PolicySet, obj_policy: np.ndarray, slot_off: Sequence[int], slot_names: Sequence[Optional[str]],
             status: np.ndarray, matched: np.ndarray) -> list:
    """Per object its overrides map — cluster name → the patches of the matched rules in rule order, the
    first policy's rules before the second's, clusters without patches left out — or the
    :class:`OverrideError` of the policy that failed. ``slot_off[i] .. slot_off[i + 1]`` are object i's rows
    of ``matched`` and ``slot_names`` the clusters they stand for (None: not a cluster of the snapshot)."""
    out = []
    op = np.asarray(obj_policy).reshape(-1, 2)
    cache: Dict[int, List[OverridePatch]] = {}
    for i in range(len(op)):
        if status[i]:
            pol = pset.policies[int(op[i][int(status[i]) - 1])]
            out.append(OverrideError(PARSE_FAILED, pol.key(), f"failed to parse overrides from {pol.kind()} {pol.key()!r}"))
            continue
        rules = [r for p in op[i] if p >= 0 for r in range(pset.pol_rule_off[p], pset.pol_rule_off[p + 1])]
        m: OverridesMap = {}
        for s in range(int(slot_off[i]), int(slot_off[i + 1])):
            name = slot_names[s]
            if name is None:
                continue
            patches: List[OverridePatch] = []
            for j, r in enumerate(rules):
                if (int(matched[s][j >> 5]) >> (j & 31)) & 1:
                    if r not in cache:
                        cache[r] = _patches(pset.rules[r])
                    patches += cache[r]
            if patches:
                m[name] = patches
        out.append(m)
    return out


class OverrideMatcher:
    """Objects, policies and clusters in; per object the overrides map or the error out — the reference's
    reconcile from lookForMatchedPolicies to mergeOverrides, its (rule, cluster) matching on the device."""

    def __init__(self, ctx, snap: Snapshot, policies: Sequence[OverridePolicy]):
        self.ctx, self.snap = ctx, snap
        self.pset = PolicySet(snap, policies)
        self.by_key = {p.key(): p for p in policies if p.namespace}
        self.cluster_by_name = {p.name: p for p in policies if not p.namespace}
        ctx.upload_override_policies(self.pset)

    def match(self, objs: Sequence[dict], is_namespaced: Sequence[bool], placed: Sequence[Sequence[str]]) -> list:
        n = len(objs)
        res: list = [None] * n
        op = np.full((n, 2), -1, np.int32)
        for i, obj in enumerate(objs):
            found, recheck, err = look_for_matched_policies(obj, is_namespaced[i], self.by_key, self.cluster_by_name)
            if err is not None:
                res[i] = OverrideError(MATCH_FAILED, None, err, recheck)
                continue
            for p in found:
                op[i][1 if p.namespace else 0] = self.pset.policy_index(p)
        off = np.zeros(n + 1, np.int32)
        off[1:] = np.cumsum([0 if res[i] is not None else len(placed[i]) for i in range(n)])
        names = [c for i in range(n) if res[i] is None for c in placed[i]]
        ids = np.array([self.snap.name_id.get(c, -1) for c in names], np.int32)
        status, matched = self.ctx.override_match(op, (off, ids), rule_words=self.pset.rule_words(op))
        slot_names = [c if k >= 0 else None for c, k in zip(names, ids)]
        maps = assemble(self.pset, op, off, slot_names, status, matched)
        return [res[i] if res[i] is not None else maps[i] for i in range(n)]


# ------------------------------------------------------------------- apply
def overrides_equal(a: Optional[OverridesMap], b: Optional[OverridesMap]) -> bool:
    """equality.Semantic.DeepEqual on two OverridesMaps (nil and empty maps / slices are equal)."""
    a, b = a or {}, b or {}
    if set(a) != set(b):
        return False
    return all(list(a[k] or []) == list(b[k] or []) for k in a)


def apply(obj: dict, overrides: Optional[OverridesMap]) -> bool:
    """The object half of reconcile (overridepolicy_controller.go:328-342): compare with the overrides the
    object holds under the override controller's name and set the new ones when they differ → needs update."""
    current = O.get_overrides(obj, PREFIXED_CONTROLLER_NAME)
    if overrides_equal(overrides, current):
        return False
    O.set_overrides(obj, PREFIXED_CONTROLLER_NAME, {c: list(p) for c, p in (overrides or {}).items()})
    return True
