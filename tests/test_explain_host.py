"""Host side of the filter diagnosis (no GPU): the exported symbol, the framework's filter order, the message."""
import ctypes

import numpy as np

from kubeadmiral_amd import build, runtime
from kubeadmiral_amd import framework as F
from kubeadmiral_amd.results import FilterDiagnosis


def test_library_exports_kad_explain():
    build.build()
    lib = ctypes.CDLL(runtime.LIB_PATH)
    assert hasattr(lib, "kad_explain") and hasattr(lib, "kad_explain_timing")
    assert {"kad_explain", "kad_explain_timing"} <= set(runtime.declared_functions())
    assert ctypes.sizeof(runtime.ExplainView) == 4 * ctypes.sizeof(ctypes.c_void_p)


def test_filter_order_follows_enabled_plugins():
    assert F.Framework().filter_order() == [0, 1, 2, 3, 4]
    fwk = F.Framework(F.EnabledPlugins([F.ClusterAffinity, F.ClusterResourcesFit, F.APIResources], [], [], []))
    assert fwk.filter_order() == [4, 2, 0]
    assert sum(1 << p for p in fwk.filter_order()) == fwk.filter_mask
    assert F.Framework(F.EnabledPlugins()).filter_order() == []
    # a SchedulingProfile that disables a filter and re-enables it moves it to the end (profile.go:62-82)
    ep = F.apply_profile(F.default_enabled_plugins(), {"filter": {"disabled": [F.APIResources],
                                                                  "enabled": [F.APIResources]}})
    assert F.Framework(ep).filter_order() == [1, 2, 3, 4, 0]


def _diag(rejected, feasible, fit, order, C=65):
    return FilterDiagnosis(np.arange(len(feasible), dtype=np.int32), np.array(rejected, np.int32),
                           np.array(feasible, np.int32), None if fit is None else np.array(fit, np.int32), None,
                           order, C)


def test_message():
    d = _diag([[13, 12, 9, 0, 31], [0, 0, 0, 0, 0], [0, 0, 65, 0, 0], [0, 0, 0, 0, 0]], [0, 65, 0, -1],
              [[3, 8, 1], [0, 0, 0], [0, 65, 0], [0, 0, 0]], [4, 1, 2, 3, 0])
    assert d.message(0) == ("0/65 clusters are available: 31 ClusterAffinity, 12 TaintToleration, "
                            "9 ClusterResourcesFit (cpu 3, memory 8, scalar 1), 13 APIResources")
    assert d.message(1) == "65/65 clusters are available"
    assert d.message(2) == "0/65 clusters are available: 65 ClusterResourcesFit (memory 65)"
    assert "sticky" in d.message(3)
    # the framework's order decides the order of the parts; without fit_detail no parenthesis
    e = _diag([[13, 12, 9, 0, 31]], [0], None, [0, 1, 2, 3, 4])
    assert e.message(0) == ("0/65 clusters are available: 13 APIResources, 12 TaintToleration, "
                            "9 ClusterResourcesFit, 31 ClusterAffinity")
