"""The inputs of test_gpu_boundaries.py reach the edges they are meant to pin, judged on the C oracle alone.

A parity test passes trivially when no unit touches the boundary, so for the C sweep (a), the exact
feasible-list lengths (d) and C = 65535 (f) the oracle's own results must put a cluster on the last live
lane (id C-1) and on the first lane of the last chunk (id 64 * (nch - 1)), hold a row of all C clusters,
and mix scheduled units with units that have no feasible cluster. No GPU is involved.
"""

import numpy as np
import pytest

import gpu_util as G
from kubeadmiral_amd import framework as F
from kubeadmiral_amd import pack


def selected_ids(res):
    """The cluster ids any unit's result row holds."""
    W = len(res.status)
    idx = np.arange(len(res.cluster))
    row = np.clip(np.searchsorted(res.out_off, idx, side="right") - 1, 0, max(0, W - 1))
    used = (idx - res.out_off[row]) < res.count[row] if W else np.zeros(len(idx), bool)
    return set(np.unique(res.cluster[used]).tolist())


def assert_reaches_edges(res, C):
    ids = selected_ids(res)
    assert C - 1 in ids, "no unit selects the last cluster"
    assert 64 * (G.nch_of(C) - 1) in ids, "no unit selects the first cluster of the last chunk"
    assert max(ids) < C
    assert (res.count == C).any(), "no unit selects every cluster"


@pytest.mark.parametrize("which", G.SWEEP_PROFILES)
@pytest.mark.parametrize("C", G.SWEEP_CS)
def test_sweep_inputs_reach_the_edges(C, which):
    """(a): under each of the three profiles. With no plugin enabled ("none") no filter runs, so no unit can be
    left without a feasible cluster: there every unit the oracle schedules must hold all C clusters instead."""
    snap, batch, fwk, res = G.sweep_case(C, which)
    assert batch.W == G.SWEEP_W + 4 and len(snap.names) == C
    assert_reaches_edges(res, C)
    ok = (res.status == pack.ST_OK) & (res.count > 0)
    assert int(ok.sum()) >= 10
    if which == "none":
        assert not fwk.enabled.filter_plugins and not fwk.enabled.select_plugins
        assert (res.count[ok] == C).all() and not (res.status == pack.ST_NO_FEASIBLE).any()
    else:
        assert int((res.status == pack.ST_NO_FEASIBLE).sum()) >= 5
    # the probes: all C clusters for the unconstrained unit, one cluster each on the edges where placement filters
    last, chunk, first, every = (res.row(G.SWEEP_W + i) for i in range(4))
    assert [c for c, _ in every[1]] == list(range(C))
    if F.PlacementFilter in fwk.enabled.filter_plugins:
        assert [c for c, _ in last[1]] == [C - 1] and [c for c, _ in chunk[1]] == [64 * (G.nch_of(C) - 1)]
        assert [c for c, _ in first[1]] == [0]


@pytest.mark.parametrize("C", G.LIST_CS)
def test_list_inputs_have_exact_lengths_and_straddles(C):
    """(d): a placement-only Duplicate unit over n clusters has n feasible clusters, so MaxCluster
    (max_cluster.go:42-66) leaves n of them without MaxClusters and min(n, MaxClusters) otherwise — none for
    MaxClusters = 0 (the n - 1 of n = 1) — and a unit with n = 0 has no feasible cluster. On each side of the
    256 and of the 512 cut some unit's selection cuts a run of tied totals (RF_TIE_STRADDLE)."""
    snap, batch, fwk, res, meta = G.list_case(C)
    assert batch.W == len(meta) == 3 * len(G.list_ns(C))
    assert_reaches_edges(res, C)
    for w, (n, maxc) in enumerate(meta):
        want = 0 if n == 0 else (n if maxc is None else min(n, maxc))
        assert int(res.count[w]) == want, (w, n, maxc)
        assert int(res.status[w]) == (pack.ST_NO_FEASIBLE if n == 0 else pack.ST_OK), (w, n, maxc)
    ns = np.array([n for n, _ in meta])
    straddle = (res.flags & pack.RF_TIE_STRADDLE) != 0
    for side in (ns <= 256, (ns > 256) & (ns <= 512), ns > 512):  # the kernels cut at n > 256 and n > 512
        assert straddle[side].any()


def test_max_c_inputs_reach_the_edges():
    """(f): C = 65535, ids up to 65534 = 0xFFFE in the results."""
    snap, batch, fwk, res = G.max_c_case()
    assert len(snap.names) == G.MAX_C and batch.W == 12
    assert_reaches_edges(res, G.MAX_C)


def test_zero_c_inputs_have_no_feasible_cluster():
    """(f): C = 0, no cluster to be feasible."""
    snap, batch, fwk, res = G.zero_c_case()
    assert len(snap.names) == 0 and batch.W == 4
    assert (res.status == pack.ST_NO_FEASIBLE).all() and not res.count.any()
