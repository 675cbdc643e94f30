"""CPU: host-side logic of the drop-in layer that needs no GPU (engine cache lifetime, option plumbing)."""
import gc
import types

import numpy as np
import pytest


class _FakeEngine:
    made = 0
    closed = []

    def __init__(self, tag):
        self.tag = tag
        _FakeEngine.made += 1

    def close(self):
        _FakeEngine.closed.append(self.tag)


def test_engine_cache_is_keyed_by_live_object_and_evicts(monkeypatch):
    """engines were cached under id(sys) with no reference to sys, so a recycled id handed a NEW System the OLD topology and
    every System leaked its HBM.  Now: weak reference + identity check + finalizer that DROPS the cache entry.  ADVICE r2: the finalizer
    must not close engines -- a caller may still hold one; an engine frees its HBM when its own last reference dies."""
    from phoskintime_amd.global_model import simulate as gsim
    monkeypatch.setattr(gsim.NetworkEngine, "from_system", classmethod(lambda cls, sys, model, device=None: _FakeEngine((sys.name, model))))
    gsim._engines.clear(); _FakeEngine.made = 0; _FakeEngine.closed.clear()

    class Sys:                                   # weak-referenceable stand-in for global_model.network.System
        def __init__(self, name):
            self.name = name

    a = Sys("a")
    e0 = gsim.engine_for(a, 0)
    assert gsim.engine_for(a, 0) is e0 and _FakeEngine.made == 1            # cached
    e2 = gsim.engine_for(a, 2)
    assert e2 is not e0 and e2.tag == ("a", 2)                             # one engine per kinetic model
    key = id(a)
    del a; gc.collect()
    assert key not in gsim._engines and _FakeEngine.closed == []           # evicted with the System; e0 / e2 are still held and stay usable
    # a stale entry under a recycled id is never handed out: simulate it by planting a dead weakref under a live object's id
    b = Sys("b")
    dead = Sys("dead"); import weakref; ref = weakref.ref(dead); del dead; gc.collect()
    stale = _FakeEngine(("stale", 0))
    gsim._engines[id(b)] = (ref, {0: stale})
    eb = gsim.engine_for(b, 0)
    assert eb.tag == ("b", 0) and gsim._engines[id(b)][1] == {0: eb}
    # objects that cannot be weakly referenced: engines live on the object itself (SimpleNamespace), or a clear error (no __dict__)
    ns = types.SimpleNamespace(name="ns")
    e_ns = gsim.engine_for(ns, 0)
    assert gsim.engine_for(ns, 0) is e_ns and ns._pk_engines == {0: e_ns} and id(ns) not in gsim._engines
    with pytest.raises(TypeError):
        gsim.engine_for(5, 0)


def test_solver_opts_kernel_field_roundtrip(built_lib):
    from phoskintime_amd import _capi
    o = _capi.default_opts()
    assert o.kernel == _capi.KERNEL_AUTO and o.method == _capi.METHOD_LRP12
    assert _capi.default_opts(kernel="tpr").kernel == _capi.KERNEL_TPR and _capi.default_opts(kernel=1).kernel == _capi.KERNEL_GROUP
    with pytest.raises(KeyError):
        _capi.default_opts(kernel="warp")


def _reference_system(g):
    """The attributes a reference ``global_model.network.System`` holds, as stored by tools/make_golden_from_system.py (which runs the
    reference's own Index / build_W_parallel / build_tf_matrix / System on the seeded network of tools/make_golden_pins.py), rebuilt
    with the reference's types: Python dicts for the index maps, arrays in the dtypes the reference keeps."""
    idx = types.SimpleNamespace(N=int(g["N"]), kinases=[str(k) for k in g["kinases"]],
                                p2i={str(k): int(v) for k, v in zip(g["p2i_keys"], g["p2i_values"])},
                                k2i={str(k): int(v) for k, v in zip(g["k2i_keys"], g["k2i_values"])},
                                offset_y=g["offset_y"], offset_s=g["offset_s"], n_sites=g["n_sites"])
    if bool(g["has_proxy_map"]):
        idx.proxy_map = {str(k): str(v) for k, v in zip(g["proxy_keys"], g["proxy_values"])}
    arrays = {k: g[k] for k in ("W_indptr", "W_indices", "W_data", "TF_indptr", "TF_indices", "TF_data", "tf_deg", "kin_grid", "kin_Kmat")}
    return types.SimpleNamespace(idx=idx, **arrays)


@pytest.mark.parametrize("model_name,m", [("distributive", 0), ("combinatorial", 2)])
def test_from_system_packs_the_real_reference_System(model_name, m):
    """a23 was only ever tested with a SimpleNamespace of made-up arrays.  Here the attributes of the REAL
    global_model.network.System (stored from a run of the reference by tools/make_golden_from_system.py: index maps, orphan -> proxy
    redirection, CSR arrays) go through NetworkEngine.desc_from_system, and the result must equal what the reference itself packs into
    odeint_args (stored in the pins fixture made from the same seeded network)."""
    from pathlib import Path
    from phoskintime_amd.global_model.engine import NetworkEngine
    golden = Path(__file__).resolve().parents[1] / "tests" / "golden"
    src = np.load(golden / f"from_system_m{m}.npz")
    assert int(src["model"]) == m and bool(src["has_proxy_map"]) and src["proxy_keys"].size >= 1, model_name
    got = NetworkEngine.desc_from_system(_reference_system(src)); want = np.load(golden / f"pins_network_m{m}.npz")
    for k in ("offset_y", "offset_s", "n_sites", "W_indptr", "W_indices", "W_data", "TF_indptr", "TF_indices", "TF_data", "tf_deg", "driver_map",
              "kin_grid", "kin_Kmat"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    assert got["driver_map"].dtype == np.int32 and (got["driver_map"] >= 0).sum() >= 2
