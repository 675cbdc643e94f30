"""CPU: the slab route of the network sensitivity launches at the surface -- ``pk_network_sens_hbm_columns`` and
``pk_network_sens_workspace_bytes`` are declared in include/phoskin.h, listed in ``_capi.SYMBOLS`` and exported; ``PK_KERNEL_HBM`` is 4 in
the header and in ``_capi``; null handles are errors (no kernel is launched here).  Both queries need a network handle, which only a GPU
makes: their arithmetic (min(K, n_var, W), the knob, slab = plain slab + the LDS kernels' sensitivity area) is held in
tests/test_gpu_network_sens_hbm.py."""
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
NEW = ("pk_network_sens_hbm_columns", "pk_network_sens_workspace_bytes")


def _header():
    return re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "phoskin.h").read_text(), flags=re.S)


def test_declared_listed_and_exported(built_lib):
    from phoskintime_amd import _capi
    txt = _header()
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", txt), name
        assert name in _capi.SYMBOLS and hasattr(built_lib, name), name


def test_kernel_value():
    from phoskintime_amd import _capi
    m = re.search(r"\bPK_KERNEL_HBM\s*=\s*(\d+)", _header())
    assert m and int(m.group(1)) == 4
    assert _capi.KERNEL_HBM == 4 and _capi.KERNELS["hbm"] == 4
    assert _capi.default_opts(kernel="hbm").kernel == 4
    # the values before it are where they were
    assert [_capi.KERNELS[k] for k in ("auto", "group", "tpr", "workspace")] == [0, 1, 2, 3]


def test_null_handles_are_errors(built_lib):
    from phoskintime_amd import _capi
    assert built_lib.pk_network_sens_hbm_columns(None, 4, 0) == _capi.PK_ERR_ARG
    assert built_lib.pk_network_sens_workspace_bytes(None, None, 1, 4, 0) == _capi.PK_ERR_ARG


def test_python_layers_exist():
    import inspect
    from phoskintime_amd.global_model import NetworkEngine
    assert callable(NetworkEngine.sens_hbm_columns) and callable(NetworkEngine.sens_workspace_bytes)
    for f in (NetworkEngine.simulate_sens_batch, NetworkEngine.simulate_objective_grad_batch):
        assert "hbm" in inspect.getdoc(f)
