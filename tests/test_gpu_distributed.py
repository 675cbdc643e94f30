"""GPU: the N > 1 code path on ONE GPU (plus, at the end, world size 2 on the real kernels with the collective on gloo) -- a fresh child process (no GPU call before init_process_group) with torch.distributed backend
"nccl" (= RCCL) at world size 1 runs the real kernels through every sharded driver: sharded_map, the network Morris driver, the
population objectives, the rows-batched LM fit, and bench.py's collective path (PK_FORCE_COLLECTIVE=1).  VERDICT r1 missing #6: no GPU
test had ever driven the nccl path.  (world size 2 of the same partition / gather logic runs on gloo in tests/test_distributed_cpu.py.)"""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]

CHILD = r'''
import os, sys, numpy as np, torch
import torch.distributed as dist
sys.path.insert(0, sys.argv[1])
os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", sys.argv[2])
os.environ.update(RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
torch.cuda.set_device(0)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
assert dist.get_backend() == "nccl"
from phoskintime_amd import batch
from phoskintime_amd.distributed import sharded_map, all_gather_replicas, all_gather_with_status, shared_seed
from oracle import protein_models as pm

# 1. per-protein kernel through sharded_map (block partition + ONE all_gather_into_tensor on the GPU)
rng = np.random.default_rng(0)
th = torch.as_tensor(rng.uniform(0.1, 3.0, (300, 12)), device="cuda")
def fn(lo, hi):
    return batch.solve_ode_batch("distmod", th[lo:hi], np.ones(6), 4, pm.TIME_POINTS, want_sol=False, want_flat=False, metric="total_signal").metric
full = sharded_map(fn, 300)
direct = batch.solve_ode_batch("distmod", th, np.ones(6), 4, pm.TIME_POINTS, want_sol=False, want_flat=False, metric="total_signal").metric
assert full.is_cuda and torch.equal(full, direct)
# the collective itself at world size 1 (all_gather_replicas short-circuits there): what N > 1 ranks execute
buf = torch.empty(300, dtype=torch.float64, device="cuda")
dist.all_gather_into_tensor(buf, direct.contiguous()); torch.cuda.synchronize()
assert torch.equal(buf, direct)
assert shared_seed(None) is None and shared_seed(3) == 3
v, st = all_gather_with_status(direct, torch.zeros(300, dtype=torch.int32, device="cuda"), 300)
assert torch.equal(v, direct) and not st.any()

# 2. network Morris driver + population objectives on a golden network
from phoskintime_amd.global_model import NetworkEngine
from phoskintime_amd.global_model.sensitivity import run_sensitivity_batch
from phoskintime_amd.global_model.optproblem import GlobalODEBatch
g = np.load(os.path.join(sys.argv[1], "tests", "golden", "pins_network_m0.npz"))
eng = NetworkEngine.from_npz(g)
keys = ("c_k", "A_i", "B_i", "C_i", "D_i", "Dp_i", "E_i", "tf_scale")
sl = {k: slice(int(a), int(b)) for k, (a, b) in zip(keys, g["slice_bounds"])}
row = g["X_phys"][2]
fitted = {k: (row[sl[k]] if k != "tf_scale" else float(row[sl[k]][0])) for k in keys}
out = run_sensitivity_batch(eng, fitted, g["tp"], g["tr"], g["tph"], trajectories=3, num_levels=8, seed=None)
D = eng.n_var
assert out["Y"].shape == (3 * (D + 1),) and not out["status"].any() and np.isfinite(out["Si"]["mu_star"]).all()
ld = {k[3:]: g[k] for k in g.files if k.startswith("ld_")}
drow = g["ev_defaults"]
defaults = {k: (drow[sl[k]] if k != "tf_scale" else float(drow[sl[k]][0])) for k in keys}
prob = GlobalODEBatch(eng, sl, ld, defaults, dict(zip(("protein", "rna", "phospho", "prior"), map(float, g["ev_lambdas"]))), g["times"], loss_mode=int(g["ev_loss_mode"]))
F = prob.evaluate(g["X_raw"])
np.testing.assert_allclose(F, g["ev_F"], rtol=2e-5)
prob.close(); eng.close()

# 3. rows-batched LM through the sharded entry point
from phoskintime_amd.paramest import fit_rows_sharded
n = 2
th_true = np.array([1.2, 0.4, 0.9, 0.15, 0.8, 0.3, 0.5, 0.25])
flat = batch.solve_ode_batch("distmod", th_true[None], np.ones(4), n, pm.TIME_POINTS, want_sol=False).flat[0].cpu().numpy()
P0 = np.tile(th_true, (5, 1)) * np.exp(0.3 * rng.standard_normal((5, 8)))
fit = fit_rows_sharded("distmod", n, pm.TIME_POINTS, P0, np.ones(4), flat, bounds=(np.zeros(8), np.full(8, 20.0)))
assert fit.p.shape == (5, 8) and (fit.cost < 1e-10).all(), fit.cost
dist.barrier(); torch.cuda.synchronize()
dist.destroy_process_group()
print("CHILD_OK")
'''


def _free_port():
    import socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def test_nccl_world_size_one_drives_every_sharded_driver(tmp_path):
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    env = dict(os.environ); env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, str(script), str(ROOT), str(_free_port())], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0 and "CHILD_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def test_bench_collective_path_at_world_size_one(tmp_path):
    """bench.py exactly as the driver launches it for N > 1 (RANK / WORLD_SIZE / MASTER_* in the environment), at world size 1 with the
    collective forced: the all-gather on its own HIP stream, the barrier and the max-over-ranks timing all execute.  --dump-outputs
    writes what the last timed step computed, the gathered scalars included."""
    env = dict(os.environ)
    env.update(RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), PK_FORCE_COLLECTIVE="1",
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    dump = tmp_path / "outputs"
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "3", "--full", "--no-cpu-baseline", "--no-secondary",
                        "--dump-outputs", str(dump)], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    line = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    assert line["n_gpus"] == 1 and "all-gather" in line["config"]["workload"] and line["value"] > 1e6
    assert line["solver"]["flagged_replicas"] == 0 and line["parity"]["max_band_err_vs_scipy_tight"] <= 0.1
    assert line["steps"] == 20 and line["ms_per_step"] > 0
    import numpy as np
    files = {f.stem: np.load(f) for f in dump.glob("*.npy")}
    assert {"metric", "status", "n_steps", "sol", "sol_replicas", "metric_gathered"} <= set(files)
    assert all(a.dtype == np.float64 for a in files.values()) and sum(f.stat().st_size for f in dump.glob("*.npy")) <= 64 << 20
    B = files["metric"].shape[0]
    assert B == 65536 and files["sol"].shape == (8192, 14, 32) and files["n_steps"].shape == (B, 2)
    assert np.array_equal(files["metric_gathered"], files["metric"]) and not files["status"].any() and np.isfinite(files["sol"]).all()


CHILD2 = r'''
import os, sys, numpy as np, torch
import torch.distributed as dist
sys.path.insert(0, sys.argv[1])
rank = int(sys.argv[3])
os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=sys.argv[2], RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK=str(rank))
torch.cuda.set_device(0)                       # both ranks share the one GPU of the box; the collective runs on gloo (host memory)
dist.init_process_group("gloo", rank=rank, world_size=2)
from phoskintime_amd import batch
from phoskintime_amd.distributed import sharded_map, shard_bounds
from oracle import protein_models as pm

# 1. the per-protein kernel through sharded_map: rank r integrates rows [lo, hi) on the GPU, the gathered vector equals the one-process result
rng = np.random.default_rng(0)
th = rng.uniform(0.1, 3.0, (301, 12))          # odd: the last rank's shard is short
def fn(lo, hi):
    return batch.solve_ode_batch("distmod", th[lo:hi], np.ones(6), 4, pm.TIME_POINTS, want_sol=False, want_flat=False, metric="total_signal", kernel="group").metric.cpu()
full = sharded_map(fn, 301)
direct = batch.solve_ode_batch("distmod", th, np.ones(6), 4, pm.TIME_POINTS, want_sol=False, want_flat=False, metric="total_signal", kernel="group").metric.cpu()
assert torch.equal(full, direct), float((full - direct).abs().max())
assert shard_bounds(301, 1, 2) == (151, 301)
# 1b. the interleaved partition in decreasing order of a cost proxy (VERDICT r2 item 7): rank r owns positions r, r + 2, ... of the order;
# one all-gather, global row order restored, equal to the one-process result BIT FOR BIT under the pinned kernel family
from phoskintime_amd.distributed import sharded_map_rows
thd = torch.as_tensor(th, device="cuda")
def fn_rows(rows):
    return batch.solve_ode_batch("distmod", thd[rows.cuda()], np.ones(6), 4, pm.TIME_POINTS, want_sol=False, want_flat=False, metric="total_signal", kernel="group").metric.cpu()
assert torch.equal(sharded_map_rows(fn_rows, 301, cost=torch.as_tensor(th.max(axis=1))), direct)
assert torch.equal(sharded_map_rows(fn_rows, 301), direct)

# 2. rows-batched LM (sensitivity Jacobian) through the sharded entry point against the one-process fit
from phoskintime_amd.paramest import fit_rows_sharded, fit_rows_batch
n = 2
th_true = np.array([1.2, 0.4, 0.9, 0.15, 0.8, 0.3, 0.5, 0.25])
flat = batch.solve_ode_batch("distmod", th_true[None], np.ones(4), n, pm.TIME_POINTS, want_sol=False).flat[0].cpu().numpy()
P0 = np.tile(th_true, (7, 1)) * np.exp(0.3 * rng.standard_normal((7, 8)))
kw = dict(bounds=(np.zeros(8), np.full(8, 20.0)), kernel="group")
fs = fit_rows_sharded("distmod", n, pm.TIME_POINTS, P0, np.ones(4), flat, **kw)
fb = fit_rows_batch("distmod", n, pm.TIME_POINTS, P0, np.ones(4), flat, **kw)
assert fs.p.shape == (7, 8) and (fs.cost < 1e-10).all(), fs.cost
np.testing.assert_allclose(fs.p, fb.p, rtol=1e-6, atol=1e-9)

# 3. network Morris driver with seed=None: rank 0's entropy is broadcast, both ranks build the same design and return the same Y
from phoskintime_amd.global_model import NetworkEngine
from phoskintime_amd.global_model.sensitivity import run_sensitivity_batch
g = np.load(os.path.join(sys.argv[1], "tests", "golden", "pins_network_m0.npz"))
eng = NetworkEngine.from_npz(g)
keys = ("c_k", "A_i", "B_i", "C_i", "D_i", "Dp_i", "E_i", "tf_scale")
sl = {k: slice(int(a), int(b)) for k, (a, b) in zip(keys, g["slice_bounds"])}
row = g["X_phys"][2]
fitted = {k: (row[sl[k]] if k != "tf_scale" else float(row[sl[k]][0])) for k in keys}
out = run_sensitivity_batch(eng, fitted, g["tp"], g["tr"], g["tph"], trajectories=3, num_levels=8, seed=None)
assert not out["status"].any() and np.isfinite(out["Si"]["mu_star"]).all()
both = [None, None]
dist.all_gather_object(both, (np.asarray(out["Y"]).tobytes(), np.asarray(out["param_values"]).tobytes()))
assert both[0] == both[1], "ranks disagree on the Morris design / outputs"
# ... and the interleaved rows, gathered, are what ONE process computes for the whole design, bit for bit
from phoskintime_amd.global_model.sensitivity import scalar_metric_batch
from phoskintime_amd.global_model.simulate import measure_tolerances
times = np.unique(np.concatenate([g["tp"], g["tr"], g["tph"]]).astype(np.float64))
lists, ld_ = eng.make_index_lists(times, g["tp"], g["tr"], g["tph"])
Yall, st_, _ = eng.simulate_batch(out["param_values"], times, max_steps=5000 * times.size, **measure_tolerances(eng))
pred = eng.observables_batch(lists, Yall, ld_["p_prot"].size + ld_["p_rna"].size + ld_["p_pho"].size, eps=1e-12)
one = scalar_metric_batch(pred, "total_signal").cpu().numpy()
assert np.array_equal(one, out["Y"]), "sharded Morris outputs differ from the one-process ones: %d of %d rows, max |d| %.3e, status %s" % (
    int((one != out["Y"]).sum()), one.size, float(np.nanmax(np.abs(one - out["Y"]))), st_.cpu().numpy().tolist())
eng.free_loss(lists)
eng.close()
dist.barrier()
dist.destroy_process_group()
print("CHILD2_OK", rank)
'''


def test_two_ranks_on_one_gpu_with_gloo_run_the_sharded_drivers_on_the_real_kernels(tmp_path):
    """World size 2 with the REAL kernels: both ranks use the box's one GPU (two processes on the card), the single all-gather of each
    driver runs on gloo.  Checks what world size 1 cannot: short last shard, gather order, the broadcast Morris seed, and that the sharded
    LM fit equals the one-process fit row for row."""
    script = tmp_path / "child2.py"
    script.write_text(CHILD2)
    env = dict(os.environ); env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    port = str(_free_port())
    procs = [subprocess.Popen([sys.executable, str(script), str(ROOT), port, str(r)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env) for r in (0, 1)]
    outs = []
    for p in procs:
        try:
            o, e = p.communicate(timeout=900)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append((p.returncode, o, e))
    for rc, o, e in outs:
        if not (rc == 0 and "CHILD2_OK" in o):
            pytest.fail("child rank failed (rc %d):\n%s\n%s" % (rc, o[-1000:], e[-2500:]), pytrace=False)


@pytest.mark.gpu
def test_c_abi_collective_on_a_world_of_one():
    """VERDICT r2 missing #7: the all-gather of the sharded drivers behind the C ABI (``pk_comm_unique_id / pk_comm_init / pk_allgather_f64 /
    pk_comm_destroy``, RCCL bound at run time) for embedders without torch.distributed.  One GPU here: a world of one rank goes through
    the real RCCL communicator and the real collective on the context's stream; argument errors are reported, not crashed on."""
    import ctypes as C
    import numpy as np
    import torch
    from phoskintime_amd import batch
    ctx = batch.get_context()
    lib = ctx.lib
    ident = C.create_string_buffer(128)
    ctx.check(lib.pk_comm_unique_id(ctx.handle, ident))
    assert any(ident.raw)
    assert lib.pk_comm_rank(ctx.handle) < 0                                  # no communicator yet
    ctx.check(lib.pk_comm_init(ctx.handle, ident.raw, 0, 1))
    assert lib.pk_comm_rank(ctx.handle) == 0 and lib.pk_comm_world(ctx.handle) == 1
    assert lib.pk_comm_init(ctx.handle, ident.raw, 0, 1) < 0                 # one communicator per context
    send = torch.arange(4096, dtype=torch.float64, device="cuda") * 0.5
    recv = torch.full((4096,), -1.0, dtype=torch.float64, device="cuda")
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.check(lib.pk_allgather_f64(ctx.handle, send.data_ptr(), 4096, recv.data_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(send, recv)
    # the pattern of the sharded drivers: this rank's rows of a batched solve, gathered
    from oracle import protein_models as pm
    th = np.random.default_rng(0).uniform(0.1, 3.0, (64, 12))
    out = batch.solve_ode_batch("distmod", th, np.ones(6), 4, pm.TIME_POINTS, want_sol=False, want_flat=False, metric="total_signal").metric
    got = torch.empty_like(out)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.check(lib.pk_allgather_f64(ctx.handle, out.data_ptr(), out.numel(), got.data_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(out, got)
    assert lib.pk_allgather_f64(ctx.handle, None, 4, recv.data_ptr()) < 0 and lib.pk_allgather_f64(ctx.handle, send.data_ptr(), -1, recv.data_ptr()) < 0
    ctx.check(lib.pk_comm_destroy(ctx.handle))
    assert lib.pk_allgather_f64(ctx.handle, send.data_ptr(), 4, recv.data_ptr()) < 0     # destroyed
    ctx.check(lib.pk_comm_destroy(ctx.handle))                               # idempotent
