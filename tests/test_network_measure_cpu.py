"""CPU: the C ABI of the fused network measurement (pk_network_simulate_measure_batch, include/phoskin.h) is built, exported and bound;
its argument check answers without a context.  No kernel is launched here."""
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def test_library_exports_the_symbol(built_lib):
    from phoskintime_amd import _capi
    assert "pk_network_simulate_measure_batch" in _capi.SYMBOLS
    assert hasattr(built_lib, "pk_network_simulate_measure_batch")


def test_null_context_is_an_argument_error(built_lib):
    f = built_lib.pk_network_simulate_measure_batch
    rc = f(None, None, None, 1, None, 0, None, 0, None, 1, None, 1e-12, 0, None, None, None, None, None)
    assert rc < 0


def test_metric_ids_match_the_header():
    from phoskintime_amd import _capi
    assert (_capi.NET_METRIC_TOTAL_SIGNAL, _capi.NET_METRIC_MEAN, _capi.NET_METRIC_VARIANCE, _capi.NET_METRIC_L2_NORM) == (0, 1, 2, 3)
    assert _capi.NET_METRICS == dict(total_signal=0, mean=1, variance=2, l2_norm=3)
    txt = (ROOT / "include" / "phoskin.h").read_text()
    for name, v in (("TOTAL_SIGNAL", 0), ("MEAN", 1), ("VARIANCE", 2), ("L2_NORM", 3)):
        assert re.search(rf"\bPK_NET_METRIC_{name}\s*=\s*{v}\b", txt), name
