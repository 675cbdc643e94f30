"""CPU: the two Sobol' entry points are declared in include/phoskin.h, listed in ``_capi.SYMBOLS``, exported by the library, and answer a
null context with an error code (no kernel is launched here)."""
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
NEW = ("pk_sobol_build_batch", "pk_sobol_indices_batch")


def test_declared_listed_and_exported(built_lib):
    from phoskintime_amd import _capi
    txt = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "phoskin.h").read_text(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", txt), name
        assert name in _capi.SYMBOLS and hasattr(built_lib, name), name


def test_null_context_is_an_error(built_lib):
    from phoskintime_amd import _capi
    assert built_lib.pk_sobol_build_batch(None, 4, 2, None, None, None, None, None) == _capi.PK_ERR_ARG
    assert built_lib.pk_sobol_indices_batch(None, 4, 2, 3, None, None, 0, None, None, None, None, None) == _capi.PK_ERR_ARG


def test_python_layers_exist():
    from phoskintime_amd.sensitivity import sobol, analysis
    from phoskintime_amd.global_model import sensitivity
    for f in (sobol.draw, sobol.build, sobol.sample, sobol.resample_counts, sobol.analyze, sobol.sample_device, sobol.indices_device,
              analysis.temporal_sobol_batch, sensitivity.temporal_gsa_batch):
        assert callable(f)
