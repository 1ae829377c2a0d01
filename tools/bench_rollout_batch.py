"""Batched roll-out throughput (Tennis-main 256x256, S=4, 32 frames per sequence): python tools/bench_rollout_batch.py [frames]

For n in 1, 2, 4, 8, 16: start_inference(n) + `frames` x generate_next_batch, the median of three timed roll-outs after a warm-up one (as bench.py:rollout_fps) --
aggregate frames/s, ms per step, launches per step (the two boundary kernels + the kernel nodes of the captured graph), spread, and the convolution kernel families one
frame runs on.  For comparison: n single-sequence roll-outs one after the other on the existing entry (caddy_generate_next).
The kernel families need one timed record per launch, so a child process with CADDY_ROLLOUT_GRAPH=0 (eager frames) collects them: `--families`."""
import ctypes as C
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from playablevideogeneration_amd import configs  # noqa: E402
from playablevideogeneration_amd.engine import Engine  # noqa: E402
from playablevideogeneration_amd.init import init_parameters  # noqa: E402

only_families = "--families" in sys.argv[1:]
args = [a for a in sys.argv[1:] if a != "--families"]
frames = int(args[0]) if args else 32
dev = torch.device("cuda", 0)
c = dict(configs.TENNIS)
K = c["actions"]


def engine(n):
    eng = Engine(variant=c["variant"], batch=n, seq_len=2, height=256, width=256, stacking=c["stacking"], actions=K, action_dim=c["action_dim"], hidden=c["hidden"], device=dev)
    init_parameters(eng, seed=0)
    return eng


def median_of_three(run):
    runs = []
    for rep in range(4):      # first repetition = warm-up (graph capture, caches)
        r = run()
        if rep:
            runs.append(r)
    runs.sort()
    return runs[1], (runs[-1] - runs[0]) / runs[1]


def launches_per_step(eng):
    """the two boundary kernels + the kernel nodes of the captured per-frame graph; "eager": no graph is captured, "n/a": it is, but its nodes could not be counted"""
    eng.lib.caddy_debug_rollout_graph_nodes.restype = C.c_int
    eng.lib.caddy_debug_rollout_graph_nodes.argtypes = [C.c_void_p]
    k = int(eng.lib.caddy_debug_rollout_graph_nodes(eng.ctx))
    return "eager" if k == 0 else "n/a" if k < 0 else str(k + 2)


def families(eng, step):
    """convolution kernel families of ONE frame (eager launches with HIP events around every convolution)"""
    eng.profile_begin()
    step()
    fam = eng.profile_end()
    return ", ".join(f"{name} x{v[0]} ({1e3 * v[2]:.0f} us)" for name, v in fam.items() if v[0])


torch.manual_seed(0)
obs_all = torch.rand(16, 3 * c["stacking"], 256, 256, device=dev) * 2 - 1
if only_families:
    assert os.environ.get("CADDY_ROLLOUT_GRAPH") == "0", "--families times single launches: run it with CADDY_ROLLOUT_GRAPH=0"
    print("convolution kernel families of one frame (launches, time):")
    for n in (1, 2, 4, 8, 16):
        eng = engine(n)
        obs0 = obs_all[:n].contiguous()
        acts = [s % K for s in range(n)]
        eng.start_inference(n)
        eng.generate_next_batch(obs0, acts)      # (warm-up frame)
        print(f"  n={n:>2}: {families(eng, lambda: eng.generate_next_batch(obs0, acts))}", flush=True)
        del eng
        torch.cuda.empty_cache()
    sys.exit(0)
print(f"batched roll-out, Tennis-main 256x256, S={c['stacking']}, {frames} frames per sequence, median of 3 timed roll-outs (warm-up roll-out first)")
print(f"{'n':>3} {'frames/s':>10} {'ms/step':>9} {'launches/step':>14} {'spread':>8} | {'n x single entry, frames/s':>27} {'spread':>8}")
single = engine(1)
for n in (1, 2, 4, 8, 16):
    eng = engine(n)
    obs0 = obs_all[:n].contiguous()
    acts = [[(i + s) % K for s in range(n)] for i in range(frames + 4)]

    def batched():
        obs = obs0
        eng.start_inference(n)
        for i in range(4):
            _, obs = eng.generate_next_batch(obs, acts[i])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(frames):
            _, obs = eng.generate_next_batch(obs, acts[4 + i])
        torch.cuda.synchronize()
        return n * frames / (time.perf_counter() - t0)

    def sequential():
        dt = 0.0
        for s in range(n):
            obs = obs0[s]
            single.start_inference()
            for i in range(4):
                _, obs = single.generate_next(obs, acts[i][s])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(frames):
                _, obs = single.generate_next(obs, acts[4 + i][s])
            torch.cuda.synchronize()
            dt += time.perf_counter() - t0
        return n * frames / dt

    fps, spread = median_of_three(batched)
    launches = launches_per_step(eng)
    fps1, spread1 = median_of_three(sequential)
    print(f"{n:>3} {fps:>10.1f} {1e3 * n / fps:>9.3f} {launches:>14} {100 * spread:>7.1f}% | {fps1:>27.1f} {100 * spread1:>7.1f}%", flush=True)
    del eng
    torch.cuda.empty_cache()
del single
torch.cuda.empty_cache()
sys.stdout.flush()
sys.exit(subprocess.call([sys.executable, os.path.abspath(__file__), "--families"], env=dict(os.environ, CADDY_ROLLOUT_GRAPH="0")))
