"""CPU: the network fit's entry point is declared in include/phoskin.h, listed in ``_capi.SYMBOLS``, exported by the library, and answers
a null context / handle with an error code (no kernel is launched here); the Python layers above it exist."""
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
NEW = ("pk_network_fit_batch",)


def test_declared_listed_and_exported(built_lib):
    from phoskintime_amd import _capi
    txt = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "phoskin.h").read_text(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", txt), name
        assert name in _capi.SYMBOLS and hasattr(built_lib, name), name


def test_null_handles_are_errors(built_lib):
    from phoskintime_amd import _capi
    assert built_lib.pk_network_fit_batch(None, None, None, 1, None, 0, None, 0, None, 2, None, None, 1, None, None, None, None, None, 0, None, 1e12,
                                          None, None, None, None, None, None, None) == _capi.PK_ERR_ARG


def test_python_layers_exist():
    from phoskintime_amd.global_model import NetworkEngine, polish
    from phoskintime_amd.global_model.optproblem import GlobalODEBatch
    assert callable(NetworkEngine.fit_batch) and callable(polish.polish_batch) and callable(polish.covariance)
    assert callable(GlobalODEBatch.polish)
