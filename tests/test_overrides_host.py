"""Override policies on the host: the checker (override_ref.py) and the product's lookup / merge reproduce the
reference's own test tables (tests/golden/override_policy.json, from pkg/controllers/override/util_test.go), and
a numpy interpreter of the packed policy-set blob — requirement rows from the snapshot's label columns, then
the M / E walk of include/kad_sched.h — equals the checker on those cases and on seeded fuzz, so packer and
format errors show without a GPU. The blob validator is exercised through ctypes (host code only)."""

import ctypes
import functools
import json
import os

import numpy as np
import pytest

import override_ref as R
from kubeadmiral_amd import overrides as OV
from kubeadmiral_amd import pack, synth

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "override_policy.json")) as _f:
    GOLDEN = json.load(_f)


def ids(cases):
    return [f"{c['line']}:{c['name'][:50]}" for c in cases]


# ------------------------------------------------------------------ golden
def test_fixture_counts():
    assert [len(GOLDEN[k]) for k in ("TestIsClusterMatched", "TestParseOverrides", "TestLookForMatchedPolicies",
                                     "TestMergeOverrides")] == [18, 5, 9, 3]


@pytest.mark.parametrize("case", GOLDEN["TestIsClusterMatched"], ids=ids(GOLDEN["TestIsClusterMatched"]))
def test_checker_is_cluster_matched(case):
    got = R.is_cluster_matched(R.target_from_json(case["targetClusters"]), R.cluster_from_json(case["cluster"]))
    assert got == (case["shouldMatch"], False)


@pytest.mark.parametrize("case", GOLDEN["TestParseOverrides"], ids=ids(GOLDEN["TestParseOverrides"]))
def test_checker_parse_overrides(case):
    m, err = R.parse_overrides(R.policy_from_json(case["policy"]), [R.cluster_from_json(c) for c in case["clusters"]])
    assert err == case["isErrorExpected"]
    assert m == R.map_from_json(case["expected"])


def _obj(meta):
    return {"metadata": {"namespace": meta["namespace"], "labels": dict(meta["labels"])}}


@pytest.mark.parametrize("case", GOLDEN["TestLookForMatchedPolicies"], ids=ids(GOLDEN["TestLookForMatchedPolicies"]))
def test_look_for_matched_policies(case):
    ops = {p["namespace"] + "/" + p["name"]: OV.OverridePolicy(p["name"], p["namespace"]) for p in case["overridePolicies"]}
    cops = {p["name"]: OV.OverridePolicy(p["name"], None) for p in case["clusterOverridePolicies"]}
    found, recheck, err = OV.look_for_matched_policies(_obj(case["obj"]), True, ops, cops)
    assert (err is not None) == case["isErrorExpected"]
    assert recheck == case["expectedNeedsRecheckOnError"]
    assert ([p.key() for p in found] or None if found is not None else None) == case["expectedPolicyKeys"]


def test_look_for_matched_policies_edges():
    cops = {"c": OV.OverridePolicy("c", None)}
    ops = {"ns/p": OV.OverridePolicy("p", "ns")}
    o = {"metadata": {"namespace": "ns", "labels": {OV.OVERRIDE_POLICY_NAME_LABEL: "p"}}}
    assert OV.look_for_matched_policies(o, False, ops, cops) == ([], False, None)  # cluster-scoped target: no pp
    o["metadata"]["labels"][OV.CLUSTER_OVERRIDE_POLICY_NAME_LABEL] = ""
    assert OV.look_for_matched_policies(o, True, ops, cops) == (None, False, "policy name cannot be empty")


@pytest.mark.parametrize("case", GOLDEN["TestMergeOverrides"], ids=ids(GOLDEN["TestMergeOverrides"]))
def test_merge_overrides(case):
    got = OV.merge_overrides(R.map_from_json(case["dst"]), R.map_from_json(case["src"]))
    assert got == R.map_from_json(case["expected"])


# ----------------------------------------------------- blob interpreter
def req_rows(snap, pset):
    """bool[NR][C] of the blob's requirement table from the snapshot's label columns (KAD_OP_* semantics)."""
    C = snap.C
    lval, lint, lok = snap.arrays[pack.S_LABEL_VAL], snap.arrays[pack.S_LABEL_INT], snap.arrays[pack.S_LABEL_INT_OK]
    off, words = pset.arrays[OV.O_REQ_OFF], pset.arrays[OV.O_REQ]
    rows = np.zeros((len(off) - 1, C), bool)
    for r in range(len(off) - 1):
        q = [int(x) for x in words[off[r]:off[r + 1]]]
        op, n, key, pay = q[0] & 0xff, q[0] >> 8, q[1], q[2:]
        assert len(pay) == n
        if op in (pack.OP_IN, pack.OP_EQ, pack.OP_NOTIN):
            hit = np.isin(lval[key], pay)
            rows[r] = hit if op != pack.OP_NOTIN else ~hit
        elif op in (pack.OP_EXISTS, pack.OP_DNE):
            rows[r] = (lval[key] >= 0) == (op == pack.OP_EXISTS)
        elif op in (pack.OP_GT, pack.OP_LT):
            thr = (pay[0] & 0xFFFFFFFF) | (pay[1] << 32)
            ok = (lval[key] >= 0) & (lok[key] != 0)
            rows[r] = ok & ((lint[key] > thr) if op == pack.OP_GT else (lint[key] < thr))
        elif op in (pack.OP_NAME_EQ, pack.OP_NAME_NE):
            one = np.arange(C) == key
            rows[r] = one if op == pack.OP_NAME_EQ else ~one
        else:
            rows[r] = op == pack.OP_TRUE
    return rows


def rule_rows(snap, pset):
    """(M, E) bool[R][C]: the walk kad_sched.h documents for override_rule_rows_kernel."""
    C, rows = snap.C, req_rows(snap, pset)
    _, flags, name_off, name, prog_off, prog = pset.arrays[:6]
    M, E = np.zeros((pset.R, C), bool), np.zeros((pset.R, C), bool)
    for r in range(pset.R):
        f = int(flags[r])
        if not f & OV.OVR_HAS_TARGET:
            M[r] = True
        else:
            names = np.ones(C, bool)
            if f & OV.OVR_HAS_NAMES:
                names[:] = False
                names[name[name_off[r]:name_off[r + 1]]] = True
            if f & OV.OVR_SEL_INVALID:
                E[r] = names
            else:
                P = [int(x) for x in prog[prog_off[r]:prog_off[r + 1]]]
                pc = 1 + P[0]
                live = names.copy()
                for i in P[1:pc]:
                    live &= rows[i]
                if not P[pc]:
                    M[r] = live
                    assert pc + 1 == len(P)
                else:
                    pc += 2
                    for _ in range(P[pc - 1]):
                        tf, ne, nf = P[pc:pc + 3]
                        ex, fl = P[pc + 3:pc + 3 + ne], P[pc + 3 + ne:pc + 3 + ne + nf]
                        pc += 3 + ne + nf
                        if not tf & (pack.TERM_HAS_EXPR | pack.TERM_HAS_FIELD):
                            continue
                        x = live.copy()
                        if tf & pack.TERM_HAS_EXPR:
                            if not tf & pack.TERM_EXPR_VALID:
                                E[r] |= live
                                break
                            for i in ex:
                                x &= rows[i]
                        if tf & pack.TERM_HAS_FIELD:
                            if not tf & pack.TERM_FIELD_VALID:
                                E[r] |= x
                                live &= ~x
                                continue
                            for i in fl:
                                x &= rows[i]
                        M[r] |= x
                        live &= ~x
                    else:
                        assert pc == len(P)
        if f & OV.OVR_BAD_VALUE:
            E[r] |= M[r]
    return M, E


def assert_rows_equal_checker(clusters, pols):
    snap = pack.Snapshot(clusters)
    pset = OV.PolicySet(snap, pols)
    M, E = rule_rows(snap, pset)
    r = 0
    for p in pols:
        for rule in p.rules:
            bad_value = any(R._decode(o.value)[1] for o in rule.json_patch)
            for ci, c in enumerate(clusters):
                m, e = R.is_cluster_matched(rule.target_clusters, c)
                assert (bool(M[r][ci]) and not e) == (m and not e), (p.name, r, c.name)
                assert bool(E[r][ci]) == (e or (m and bad_value)), (p.name, r, c.name)
            r += 1
    assert r == pset.R
    return pset


def test_blob_interpreter_on_golden_cases():
    for case in GOLDEN["TestIsClusterMatched"]:
        pol = OV.OverridePolicy("p", None, [OV.OverrideRule(R.target_from_json(case["targetClusters"]), [])])
        assert_rows_equal_checker([R.cluster_from_json(case["cluster"])], [pol])
    for case in GOLDEN["TestParseOverrides"]:
        assert_rows_equal_checker([R.cluster_from_json(c) for c in case["clusters"]], [R.policy_from_json(case["policy"])])


@pytest.mark.parametrize("seed,C", [(1, 1), (2, 63), (3, 65), (4, 130)])
def test_blob_interpreter_on_fuzz(seed, C):
    clusters, _ = synth.gen_fuzz(seed, W=1, C=C)
    pols = synth.gen_override_policies(seed, clusters, p_invalid=0.1) + R.special_policies(clusters)[0]
    pset = assert_rows_equal_checker(clusters, pols)
    flags = pset.arrays[OV.O_RULE_FLAGS]
    for bit in (OV.OVR_HAS_TARGET, OV.OVR_HAS_NAMES, OV.OVR_SEL_INVALID, OV.OVR_BAD_VALUE):
        assert (flags & bit).any() and not (flags & bit).all()
    assert np.diff(pset.arrays[OV.O_RULE_PROG_OFF]).max() > 64  # a program longer than one 64-word window


def test_generator_has_its_own_rng():
    clusters, units = synth.gen_fuzz(7, W=5, C=20)
    a = synth.gen_override_policies(7, clusters)
    clusters2, units2 = synth.gen_fuzz(7, W=5, C=20)
    assert a == synth.gen_override_policies(7, clusters2) and units == units2 and clusters == clusters2


# -------------------------------------------------------- blob validation
@functools.lru_cache(maxsize=None)
def _packed():
    clusters, _ = synth.gen_fuzz(3, W=1, C=65)
    snap = pack.Snapshot(clusters)
    return snap, OV.PolicySet(snap, synth.gen_override_policies(3, clusters) + R.special_policies(clusters)[0])


def _check(blob, snap):
    from kubeadmiral_amd import build, runtime
    build.build()
    L = runtime.load_library()
    blob = np.ascontiguousarray(blob)
    return L.kad_override_policies_check(blob.ctypes.data, blob.nbytes, snap.blob.ctypes.data, snap.blob.nbytes)


def _hdr(blob):
    return pack.header_of(blob, OV.OverrideHeader)


def _patched(blob, fn):
    b = blob.copy()
    h = _hdr(b)
    fn(b, h)
    hb = bytes(h)
    b[:len(hb)] = np.frombuffer(hb, np.uint8)
    return b


def _arr(b, h, a):
    return b[h.off[a]:].view(np.int32)


def test_validator_accepts_packed_set():
    snap, pset = _packed()
    assert _check(pset.blob, snap) == 0


def test_validator_rejects_truncated_blobs():
    snap, pset = _packed()
    for n in (0, 8, ctypes.sizeof(OV.OverrideHeader) - 1, ctypes.sizeof(OV.OverrideHeader), len(pset.blob) - 256):
        assert _check(pset.blob[:n].copy() if n else np.zeros(1, np.uint8)[:0], snap) == -1
    # arrays moved past the end, with a consistent total size
    for a in range(OV.O_NARRAYS):
        def move(b, h, a=a):
            h.off[a] = len(b) - 4
        if a in (OV.O_RULE_NAME, OV.O_RULE_PROG, OV.O_REQ, OV.O_POL_RULE_OFF, OV.O_RULE_FLAGS, OV.O_RULE_PROG_OFF,
                 OV.O_RULE_NAME_OFF, OV.O_REQ_OFF):
            assert _check(_patched(pset.blob, move), snap) == -1, a


def test_validator_rejects_out_of_range_ids():
    snap, pset = _packed()

    def set_word(a, i, v):
        def f(b, h):
            _arr(b, h, a)[i] = v
        return f
    name_i = 0
    prog = pset.arrays[OV.O_RULE_PROG]
    prog_off = pset.arrays[OV.O_RULE_PROG_OFF]
    r_sel = next(r for r in range(pset.R) if prog[prog_off[r]] > 0)  # a rule with a selector id
    bad = [set_word(OV.O_RULE_NAME, name_i, snap.C), set_word(OV.O_RULE_NAME, name_i, -1),
           set_word(OV.O_RULE_PROG, int(prog_off[r_sel]) + 1, pset.arrays[OV.O_REQ_OFF].size - 1),  # id == NR
           set_word(OV.O_RULE_PROG, int(prog_off[r_sel]), 1 << 20),                                   # n_sel too long
           set_word(OV.O_REQ, 0, 99),                                                                 # unknown op
           set_word(OV.O_REQ, 1, 1 << 20),                                                            # label key
           set_word(OV.O_POL_RULE_OFF, 1, -5), set_word(OV.O_RULE_PROG_OFF, 1, 1 << 28),
           set_word(OV.O_RULE_FLAGS, 0, 1 << 9), set_word(OV.O_POL_RULE_OFF, pset.P, pset.R + 1)]
    # the two offset arrays the list above leaves out: a decrease, and a start other than 0 (the twin of each is
    # the packed set itself, test_validator_accepts_packed_set)
    for a in (OV.O_RULE_NAME_OFF, OV.O_REQ_OFF):
        bad += [set_word(a, 1, -1), set_word(a, 0, 1)]
    for f in bad:
        assert _check(_patched(pset.blob, f), snap) == -1


def test_validator_rejects_other_snapshot():
    snap, pset = _packed()
    other = pack.Snapshot(synth.gen_fuzz(4, W=1, C=65)[0])
    assert other.fingerprint != snap.fingerprint
    assert _check(pset.blob, other) == -1

    def fp(b, h):
        h.snapshot_fingerprint ^= 1
    assert _check(_patched(pset.blob, fp), snap) == -1


# ------------------------------------------------------- assembly, apply
def test_assemble_and_apply_from_checker_bits():
    clusters, _ = synth.gen_fuzz(5, W=1, C=20)
    pols = synth.gen_override_policies(5, clusters)
    snap = pack.Snapshot(clusters)
    pset = OV.PolicySet(snap, pols)
    rng = np.random.default_rng(5)
    cp = [i for i, p in enumerate(pols) if not p.namespace]
    npol = [i for i, p in enumerate(pols) if p.namespace]
    n = 60
    op = np.array([[cp[int(rng.integers(len(cp)))] if rng.random() < 0.7 else -1,
                    npol[int(rng.integers(len(npol)))] if rng.random() < 0.7 else -1] for _ in range(n)], np.int32)
    placed = [list(rng.choice(len(clusters), int(rng.integers(0, 6)), replace=False)) for _ in range(n)]
    off = np.zeros(n + 1, np.int32)
    off[1:] = np.cumsum([len(p) for p in placed])
    ids_ = np.array([c for p in placed for c in p], np.int32)
    rw = pset.rule_words(op)
    status, matched = R.expected_match(pols, op, off, ids_, clusters, rw)
    got = OV.assemble(pset, op, off, [clusters[c].name for c in ids_], status, matched)
    seen_err = seen_map = False
    for i in range(n):
        chain = [pols[p] for p in op[i] if p >= 0]
        want, fail_at = R.merged_overrides(chain, [clusters[c] for c in placed[i]])
        if fail_at >= 0:
            assert got[i] == OV.OverrideError(OV.PARSE_FAILED, chain[fail_at].key(), "")
            seen_err = True
            continue
        assert got[i] == want
        seen_map |= bool(want)
        obj = {"spec": {}}
        assert OV.apply(obj, got[i]) == bool(want)
        assert OV.apply(obj, got[i]) is False  # now equal to what the object holds
        from kubeadmiral_amd import objects as O
        assert OV.overrides_equal(O.get_overrides(obj, OV.PREFIXED_CONTROLLER_NAME), want)
    assert seen_err and seen_map
