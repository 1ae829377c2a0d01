"""Per-kernel parity cases of csrc/head.hip (action-network tail, sampling, centroid EMA, variations, their backward, the loss kernels, the loss finalisation, the logging
diagnostics and the per-frame evaluation sums), shared by tests/test_head_emu.py (host simulator) and tests/test_head_gpu.py (MI355X).  Every case takes (lib, dev).

Reference: a plain torch restatement with autograd (oracle/caddy_oracle.py where it states the operation), evaluated on the same float32 inputs twice: in float64 (`ref64`) and in
float32 (`ref32`).  Allowed error of a compared tensor, derived at run time (check()):

    max(8 * max|ref32 - ref64|, 16 * 2**-23 * max|ref64|)

The first term scales with the conditioning of the quantity (8: the device's expf / logf / division at a few ulp each, another summation order), the second is a floor for what
float32 torch happens to get exactly.  Exact results (arg-max, one-hot samples, zero pads, untouched buffers, planted ties) are compared exactly.  Accumulating outputs are checked
for their value on a zero base and for the accumulation on a non-zero base with 2**-23 * |base| added to the allowed error.  The conditions on the inputs (no arg-max or sign flip
within the float32 error, no L1 difference / variance / joint-matrix entry at a branch point) are asserted from ref64: a seed that misses one fails, it is never skipped.

Worst observed error / allowed per case group (every check prints its own figure; run with -s):

    group             simulator   MI355X
    head_forward      0.34        0.35
    head_backward     0.41        0.44
    loss_small        0.28        0.66 (*)
    loss_l1           0.11        0.11
    loss_mse          0.17        0.17
    diff_per_frame    0.007       0.007
    loss_finalize     0           0
    head_softmax      0.13        0.13
    loss_diagnostics  0.04        0.04

(*) d_logits_r of the (K, Da, B, T) = (3, 1, 2, 2) case with the EMA matrix: six values of at most 4e-3, what is left of logarithm terms of order one after the soft-max
    Jacobian and the factor ema_alpha; float32 torch gets them almost exactly, so the floor term is the allowed error (8.0e-9) and the device's logf leaves 5.3e-9.  The next
    figure of the group on the MI355X is 0.40 (the mutual-information loss itself).
"""
import ctypes as C

import numpy as np
import torch
import torch.nn.functional as F

from oracle import caddy_oracle as O
from playablevideogeneration_amd import _lib as L
from playablevideogeneration_amd._lib import TV
from tests.kernel_cases import P, stream, sync

U = 2.0 ** -23
WORST = {}      # group -> worst error / allowed seen by this process


def f32(x):
    """the float32 value a `float` kernel argument takes: both restatements use it, so the rounding of a constant is no error"""
    return float(np.float32(x))


def check_structs(lib):
    L.check_head_structs(lib)


def declare(lib):
    """argtypes of the entry points that take floating-point scalars by value (ctypes would pass a Python float as a double, and an int pointer as a C int)"""
    V, I, D, Fl = C.c_void_p, C.c_int, C.c_double, C.c_float
    lib.caddy_k_loss_l1.argtypes = [V, V, V, I, I, I, I, Fl, V, V, V]
    lib.caddy_k_loss_mse.argtypes = [V, V, V, Fl, V, V]
    lib.caddy_k_loss_finalize.argtypes = [V, V, D, D, D, D, D, V, V]
    lib.caddy_k_loss_small.argtypes = [V, L.ALLREDUCE_HOOK, V, V]
    lib.caddy_k_head_sample.argtypes = [V, V, V, I, V, L.ALLREDUCE_HOOK, V, V, V]
    lib.caddy_k_head_forward.argtypes = [V, V, I, I, V]
    lib.caddy_k_head_backward.argtypes = [V, V, V, I, I, I, V]
    lib.caddy_k_head_softmax.argtypes = [V, V, V, I, I, V]
    lib.caddy_k_loss_diagnostics.argtypes = [V, V, V, V]
    lib.caddy_k_loss_diff_per_frame.argtypes = [V, I, I, V, I, I, I, V, V]
    lib.caddy_k_loss_report_flag.argtypes = [V, I, V, V, V]
    return lib


NO_HOOK = L.ALLREDUCE_HOOK()      # null function pointer


def allowed(ref32, ref64, extra=0.0):
    r64 = ref64.double()
    return max(8.0 * (ref32.double() - r64).abs().max().item(), 16.0 * U * r64.abs().max().item()) + extra


def check(group, name, got, ref32, ref64, extra=0.0):
    got = got.detach().cpu().double().reshape(ref64.shape)
    assert torch.isfinite(got).all(), f"{group} {name}: non-finite values"
    err = (got - ref64.double()).abs().max().item()
    tol = allowed(ref32.detach(), ref64.detach(), extra)
    ratio = err / tol if tol > 0 else (0.0 if err == 0 else float("inf"))
    WORST[group] = max(WORST.get(group, 0.0), ratio)
    print(f"[{group}] {name}: error {err:.3e}  allowed {tol:.3e}  ratio {ratio:.3f}")
    assert err <= tol, f"{group} {name}: error {err:.3e} > allowed {tol:.3e}"


def exact(name, got, want):
    assert torch.equal(got.detach().cpu(), want.detach().cpu()), f"{name}: not exactly equal"


def flat_tv(t, N, H, W, Cc, sn, ld, off=0):
    v = TV(t.data_ptr() + 4 * off, N, H, W, Cc, sn, ld)
    v._keep = t
    return v


# ====================================================================================================================================================================================
# action head: head_forward -> head_sample -> head_backward
# ====================================================================================================================================================================================
HEAD_CASES = [
    # (B, T, F, Da, K): T = 2, one block, every loop runs once
    dict(shape=(3, 2, 5, 1, 3), seed=0, mode=1, hard=0, use_variations=1, training=1, first_call=1),
    dict(shape=(3, 2, 5, 1, 3), seed=1, mode=0, hard=0, use_variations=0, training=0, first_call=0),
    # the reference configuration; straight-through hard Gumbel; a second backward that must add
    dict(shape=(16, 9, 128, 2, 7), seed=0, mode=1, hard=1, use_variations=1, training=1, first_call=1, second_backward=True),
    dict(shape=(16, 9, 128, 2, 7), seed=1, mode=1, hard=0, use_variations=1, training=1, first_call=0),
    # K + Da = 16 fills the auxiliary row; NS = 280 > 256: strided single-block loops; NS, NT no multiples of 64 (lane loops of k_head_bwd3); odd F
    dict(shape=(40, 8, 33, 8, 8), seed=2, mode=0, hard=0, use_variations=1, training=1, first_call=1),
    dict(shape=(40, 8, 33, 8, 8), seed=5, mode=1, hard=1, use_variations=1, training=0, first_call=1, hook=True),      # (the hook is not called in evaluation mode)
    dict(shape=(5, 14, 64, 3, 5), seed=0, mode=2, hard=0, use_variations=1, training=0, first_call=1),
    dict(shape=(5, 14, 64, 3, 5), seed=1, mode=1, hard=0, use_variations=1, training=1, first_call=1, variations_in=True, hook=True),
    dict(shape=(5, 14, 64, 3, 5), seed=2, mode=0, hard=0, use_variations=1, training=1, first_call=0),
    # K = 1
    dict(shape=(2, 5, 20, 4, 1), seed=0, mode=1, hard=1, use_variations=0, training=1, first_call=1),
    dict(shape=(2, 5, 20, 4, 1), seed=1, mode=0, hard=0, use_variations=1, training=1, first_call=1),
]
TAU, ALPHA = f32(0.7), f32(0.1)


def head_inputs(B, T, Fd, Da, K, seed):
    g = torch.Generator().manual_seed(1000 + seed)
    NT, NS = B * T, B * (T - 1)
    r = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
    x = dict(feat=r(NT, Fd), Wm=r(Da, Fd) / Fd ** 0.5, bm=0.1 * r(Da), Wv=r(Da, Fd) / Fd ** 0.5, bv=0.1 * r(Da), Wf=r(K, Da), bf=0.1 * r(K),
             eps_s=r(NT, Da), eps_d=r(NS, Da), unif=torch.rand(NS, K, generator=g), cen=0.5 * r(K, Da), variations_in=r(NS, Da),
             g_logits=r(NS, K), g_ddist=r(NS, 2, Da), g_sdist=r(NT, 2, Da), g_aux=r(NS, L.AUX_LD))
    x["samples_in"] = F.one_hot(torch.randint(0, K, (NS,), generator=g), K).float()      # what an evaluation action sampler supplies
    return x


def head_ref(dt, x, B, T, Fd, Da, K, *, mode, hard, use_variations, training, first_call, variations_in=False, **_):
    """action_network.py:86-118, gumbel_softmax.py:25-72, centroid_estimator.py:38-94 as the oracle states them (Oracle.action_net / gumbel / update_centroids / variations)"""
    NS = B * (T - 1)
    t = {k: v.to(dt) for k, v in x.items()}
    leaves = {k: t[k].clone().requires_grad_(True) for k in ("feat", "Wm", "bm", "Wv", "bv", "Wf", "bf")}
    feat = leaves["feat"]
    mu = F.linear(feat, leaves["Wm"], leaves["bm"])
    raw = F.linear(feat, leaves["Wv"], leaves["bv"])
    var = raw.abs()
    sdist = torch.stack([mu, var], dim=1)
    ssamp = t["eps_s"] * torch.sqrt(var) + mu
    mu_f, var_f = mu.view(B, T, Da), var.view(B, T, Da)
    dmu, dvar = (mu_f[:, 1:] - mu_f[:, :-1]).reshape(NS, Da), (var_f[:, 1:] + var_f[:, :-1]).reshape(NS, Da)
    ddist = torch.stack([dmu, dvar], dim=1)
    dirs = t["eps_d"] * torch.sqrt(dvar) + dmu
    logits = F.linear(dirs, leaves["Wf"], leaves["bf"])
    logits.retain_grad()
    logp, prob = torch.log_softmax(logits, 1), torch.softmax(logits, 1)
    cen = t["cen"]
    if training:      # Oracle.update_centroids
        est = (dmu.unsqueeze(1) * prob.unsqueeze(-1)).sum(0) / prob.sum(0).unsqueeze(-1)
        cen = (cen * (1 - ALPHA) + est * ALPHA).detach()
    if mode == 2:
        y = t["samples_in"]
    elif mode == 1:   # Oracle.gumbel
        gum = -torch.log(-torch.log(t["unif"] + 1e-20) + 1e-20)
        y = torch.softmax((logp + gum) / TAU, dim=-1)
    else:
        y = prob
    samples = y
    if mode == 1 and hard:      # (yh - y).detach() + y, written so that the VALUE is the exact one-hot row
        yh = torch.zeros_like(y).scatter_(1, y.argmax(dim=-1, keepdim=True), 1.0)
        samples = yh + (y - y.detach())
    if variations_in:
        v = t["variations_in"]
    else:             # Oracle.variations
        v = (samples.unsqueeze(-1) * (dirs.unsqueeze(1) - cen)).sum(1)
        if not use_variations:
            v = v * 0
    loss = (logits * t["g_logits"]).sum() + (ddist * t["g_ddist"]).sum() + (sdist * t["g_sdist"]).sum()
    if first_call and mode != 2:      # externally supplied samples exist in evaluation only (model.py:171-174), where nothing is back-propagated: the head defines the
        loss = loss + (samples * t["g_aux"][:, :K]).sum() + (v * t["g_aux"][:, K:K + Da]).sum()      # auxiliary row as carrying no gradient in that mode
    loss.backward()
    out = dict(mu=mu, raw=raw, sdist=sdist, ssamp=ssamp, ddist=ddist, dirs=dirs, logits=logits, logp=logp, prob=prob, ysoft=y, samples=samples, variations=v, cen=cen)
    out = {k: a.detach() for k, a in out.items()}
    out["selected"] = y.argmax(dim=1)
    grads = dict(d_feat=leaves["feat"].grad, dWm=leaves["Wm"].grad, dbm=leaves["bm"].grad, dWv=leaves["Wv"].grad, dbv=leaves["bv"].grad, dWf=leaves["Wf"].grad,
                 dbf=leaves["bf"].grad, d_logits=logits.grad)
    return out, grads


def head_case(lib, dev, *, shape, seed, second_backward=False, hook=False, **cfg):
    """hook: an all-reduce stand-in over two identical ranks doubles the centroid sums between the two sampling kernels (training mode only): the same centroids"""
    declare(lib)
    B, T, Fd, Da, K = shape
    NT, NS = B * T, B * (T - 1)
    x = head_inputs(B, T, Fd, Da, K, seed)
    o64, g64 = head_ref(torch.float64, x, B, T, Fd, Da, K, **cfg)
    o32, g32 = head_ref(torch.float32, x, B, T, Fd, Da, K, **cfg)
    # conditions on the inputs (asserted, never skipped)
    if K > 1:
        top = o64["ysoft"].topk(2, dim=1).values
        assert (top[:, 0] - top[:, 1]).min().item() >= 1e-3, "arg-max gap of ysoft below 1e-3: choose another seed"
    assert torch.equal(o64["selected"], o32["selected"])
    raw_err = (o32["raw"].double() - o64["raw"]).abs().max().item()
    assert o64["raw"].abs().min().item() >= 100 * raw_err, f"min|raw| {o64['raw'].abs().min().item():.2e} < 100 x {raw_err:.2e}: choose another seed"

    st = stream(dev)
    d = {k: v.contiguous().to(dev) for k, v in x.items()}
    junk = lambda *s: torch.full(s, 7.5, device=dev)      # noqa: E731
    b = dict(mu=junk(NT, Da), raw=junk(NT, Da), sdist=junk(NT, 2, Da), ssamp=junk(NT, Da), ddist=junk(NS, 2, Da), dirs=junk(NS, Da), logits=junk(NS, K), logp=junk(NS, K),
             prob=junk(NS, K), ysoft=junk(NS, K), samples=junk(NS, K), variations=junk(NS, Da), aux=junk(NS, L.AUX_LD), cen_used=junk(16 * 8),
             selected=torch.full((NS,), -7, dtype=torch.int64, device=dev), d_feat=junk(NT, Fd), g_dmu=junk(NS, Da), g_dvar=junk(NS, Da), g_mu=junk(NT, Da), g_raw=junk(NT, Da))
    up = dict(d_logits=d["g_logits"].clone(), d_ddist=d["g_ddist"].clone(), d_sdist=d["g_sdist"].clone(), d_aux=d["g_aux"].clone())
    pg = dict(dWm=torch.zeros(Da, Fd, device=dev), dbm=torch.zeros(Da, device=dev), dWv=torch.zeros(Da, Fd, device=dev), dbv=torch.zeros(Da, device=dev),
              dWf=torch.zeros(K, Da, device=dev), dbf=torch.zeros(K, device=dev))
    cen = d["cen"].clone()
    cen_sums = junk(16 * 8 + 16)
    hp = L.HeadParams(Fd, Da, K, *[d[n].data_ptr() for n in ("Wm", "bm", "Wv", "bv", "Wf", "bf")], *[pg[n].data_ptr() for n in ("dWm", "dbm", "dWv", "dbv", "dWf", "dbf")])
    hb = L.HeadBufs()
    for n in ("feat", "eps_s", "eps_d", "unif"):
        setattr(hb, n, d[n].data_ptr())
    for n, tns in list(b.items()) + list(up.items()):
        setattr(hb, n, tns.data_ptr())
    sc = L.SampleCfg(cfg["mode"], cfg["hard"], cfg["training"], cfg["use_variations"], TAU, ALPHA, cen.data_ptr(),
                     d["samples_in"].data_ptr() if cfg["mode"] == 2 else None, d["variations_in"].data_ptr() if cfg.get("variations_in") else None)
    assert lib.caddy_k_head_forward(C.byref(hb), C.byref(hp), B, T, st) == 0
    calls = []

    def double_in_place(ptr, count, user):
        v = TV(ptr, 1, 1, count, 1, count, 1)
        calls.append((ptr, count, lib.caddy_k_copy(C.byref(v), C.byref(v), 1, st)))
    cb = L.ALLREDUCE_HOOK(double_in_place)
    assert lib.caddy_k_head_sample(C.byref(hb), C.byref(hp), C.byref(sc), NS, P(cen_sums), cb if hook else NO_HOOK, None, None, st) == 0
    sync(dev)
    assert calls == ([(cen_sums.data_ptr(), K * Da + K, 0)] if hook and cfg["training"] else [])
    G = "head_forward"
    for n in ("mu", "raw", "sdist", "ssamp", "ddist", "dirs", "logits", "logp", "prob", "ysoft", "samples", "variations"):
        check(G, n, b[n], o32[n], o64[n])
    check(G, "cen_used", b["cen_used"][:K * Da], o32["cen"], o64["cen"])
    if cfg["training"]:
        check(G, "centroids", cen, o32["cen"], o64["cen"])
        exact("cen_used == centroids", b["cen_used"][:K * Da].reshape(K, Da), cen)
    else:
        exact("centroids untouched in evaluation mode", cen, x["cen"])
    exact("selected", b["selected"], o64["selected"])
    if (cfg["mode"] == 1 and cfg["hard"]) or cfg["mode"] == 2:
        exact("one-hot samples", b["samples"], o64["samples"].float())
    aux = b["aux"].cpu()
    exact("aux[:, :K] == samples", aux[:, :K], b["samples"])
    exact("aux[:, K:K+Da] == variations", aux[:, K:K + Da], b["variations"])
    exact("aux zero pad", aux[:, K + Da:], torch.zeros(NS, L.AUX_LD - K - Da))
    if not cfg["use_variations"] and not cfg.get("variations_in"):
        exact("variations switched off", b["variations"], torch.zeros(NS, Da))

    first = cfg["first_call"]
    assert lib.caddy_k_head_backward(C.byref(hb), C.byref(hp), C.byref(sc), B, T, first, st) == 0
    sync(dev)
    G = "head_backward"
    check(G, "d_feat", b["d_feat"], g32["d_feat"], g64["d_feat"])
    check(G, "d_logits", up["d_logits"], g32["d_logits"], g64["d_logits"])
    for n in pg:
        check(G, n, pg[n], g32[n], g64[n])
    for n in ("d_ddist", "d_sdist", "d_aux"):
        exact(n + " is an input of the backward", up[n], x["g" + n[1:]])
    if second_backward:      # parameter gradients add; d(feat) and d(logits) are recomputed from the same upstream content
        first_dfeat = b["d_feat"].clone()
        base = {n: pg[n].clone() for n in pg}
        up["d_logits"].copy_(d["g_logits"])
        assert lib.caddy_k_head_backward(C.byref(hb), C.byref(hp), C.byref(sc), B, T, first, st) == 0
        sync(dev)
        exact("d_feat of the second backward", b["d_feat"], first_dfeat)
        for n in pg:
            extra = allowed(g32[n], g64[n]) + U * base[n].abs().max().item()      # the base carries the first call's error
            check(G, n + " (second call adds)", pg[n], 2 * g32[n], 2 * g64[n], extra=extra)


def head_limits_case(lib, dev):
    """head_sample refuses what its fixed-size rows cannot hold, before any launch"""
    declare(lib)
    hb, sc = L.HeadBufs(), L.SampleCfg()
    for K, Da in ((12, 5), (17, 1), (4, 9)):      # K + Da > 16, K > 16, Da > 8
        hp = L.HeadParams(8, Da, K)
        assert lib.caddy_k_head_sample(C.byref(hb), C.byref(hp), C.byref(sc), 4, None, NO_HOOK, None, None, stream(dev)) == -1


# ====================================================================================================================================================================================
# loss_small: entropy + KL(dir || N(0, 1)) + (smooth) mutual information + KL(general gaussian), with their gradient seeds
# ====================================================================================================================================================================================
SMALL_CASES = [
    # (K, Da, B, T), mi_lamb, zero_col: the logit column set to -200 in both calls (exact zeros of the soft-max: the m < eps and row / column clamp branches, zero gradient there)
    dict(shape=(16, 8, 30, 11), lamb=1.0, seed=0),      # K x K = 256: the whole block
    dict(shape=(3, 1, 2, 2), lamb=0.5, seed=1),
    dict(shape=(1, 8, 70, 5), lamb=2.0, seed=2),
    dict(shape=(7, 2, 5, 4), lamb=2.0, seed=3, zero_col=2),
    dict(shape=(16, 3, 3, 3), lamb=0.5, seed=4, zero_col=15),
]
SMALL_W = dict(w_mi=f32(1.3), w_entropy=f32(0.7), w_dirkl=f32(0.9), w_statekl=f32(1.1))
EMA_ALPHA = f32(0.2)
FEPS = 2.220446049250313e-16


def small_inputs(K, Da, B, T, seed, zero_col=None):
    g = torch.Generator().manual_seed(2000 + seed)
    NS, NT = B * (T - 1), B * T
    r = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
    x = dict(logits=1.5 * r(NS, K), logits_r=1.5 * r(NS, K))
    if zero_col is not None:
        x["logits"][:, zero_col] = -200.0
        x["logits_r"][:, zero_col] = -200.0
    x["ddist"] = torch.stack([r(NS, Da), 0.2 + 1.5 * torch.rand(NS, Da, generator=g)], dim=1)
    lo, hi = np.log(0.004), np.log(1.0)      # variances on both sides of the 0.05 clamp
    x["sdist"] = torch.stack([r(NT, Da), torch.exp(lo + (hi - lo) * torch.rand(NT, Da, generator=g))], dim=1)
    x["sdist_r"] = torch.stack([r(NT, Da), torch.exp(lo + (hi - lo) * torch.rand(NT, Da, generator=g))], dim=1)
    e = torch.rand(K, K, generator=g) + 0.1
    if zero_col is not None:
        e[zero_col, :] = 0.0
        e[:, zero_col] = 0.0
    x["ema"] = e / e.sum()
    for n in ("sdist", "sdist_r"):
        v = x[n][:, 1]
        v[(v - 0.05).abs() < 1e-3] += 2e-3      # keep clear of the branch point
        assert (v - 0.05).abs().min().item() >= 1e-4, "state variance within 1e-4 of the clamp: choose another seed"
        assert (v < 0.05).any() and (v > 0.05).any()
    return x


def small_ref(dt, x, lamb, use_ema):
    t = {k: v.to(dt) for k, v in x.items()}
    leaves = {k: t[k].clone().requires_grad_(True) for k in ("logits", "logits_r", "ddist", "sdist", "sdist_r")}
    lg, lr = leaves["logits"], leaves["logits_r"]
    ent = O.entropy_logit_loss(lg)
    dkl = O.kl_gaussian_loss(leaves["ddist"])
    mi, new_ema = O.mutual_information_loss(torch.softmax(lg, -1), torch.softmax(lr, -1), lamb=lamb, ema=t["ema"] if use_ema else None, alpha=EMA_ALPHA)
    skl = O.kl_general_gaussian_loss(leaves["sdist_r"], leaves["sdist"].detach())
    total = SMALL_W["w_entropy"] * ent + SMALL_W["w_dirkl"] * dkl + SMALL_W["w_mi"] * mi + SMALL_W["w_statekl"] * skl
    total.backward()
    assert leaves["sdist"].grad is None      # the reference distribution is detached
    m = O.joint_matrix(torch.softmax(lg, -1), torch.softmax(lr, -1)).detach()
    if use_ema:
        m = t["ema"] * (1 - EMA_ALPHA) + m * EMA_ALPHA
    out = dict(entropy=ent.detach(), dir_kl=dkl.detach(), mi=mi.detach(), state_kl=skl.detach(), d_logits=lg.grad, d_logits_r=lr.grad, d_ddist=leaves["ddist"].grad,
               d_sdist_r=leaves["sdist_r"].grad, new_ema=new_ema, joint=m)
    return out


def small_case(lib, dev, *, shape, lamb, seed, zero_col=None, use_ema=False, update_ema=0, hook=False, base=False):
    """base: the gradient buffers start from random content (the kernel adds); hook: an all-reduce stand-in that doubles the joint matrix, with mi_grad_scale = 2 (two identical ranks)"""
    declare(lib)
    K, Da, B, T = shape
    NS, NT = B * (T - 1), B * T
    x = small_inputs(K, Da, B, T, seed, zero_col)
    r64, r32 = small_ref(torch.float64, x, lamb, use_ema), small_ref(torch.float32, x, lamb, use_ema)
    live = r64["joint"][r64["joint"] >= FEPS]
    assert live.numel() > 0 and live.min().item() >= 1e-6, "an un-clamped joint-matrix entry below 1e-6: choose another seed"
    if zero_col is not None:
        assert (r64["joint"] < FEPS).sum().item() == 2 * K - 1 and (r64["joint"].sum(1) < FEPS).sum().item() == 1
        assert r64["d_logits"][:, zero_col].abs().max().item() < 1e-60      # zero gradient in the clamped branches

    st = stream(dev)
    d = {k: v.contiguous().to(dev) for k, v in x.items()}
    p, logp, q = (torch.full((NS, K), 7.5, device=dev) for _ in range(3))
    assert lib.caddy_k_head_softmax(P(d["logits"]), P(p), P(logp), NS, K, st) == 0
    assert lib.caddy_k_head_softmax(P(d["logits_r"]), P(q), None, NS, K, st) == 0
    gb = torch.Generator().manual_seed(77)
    mk = (lambda *s: torch.randn(*s, generator=gb).to(dev)) if base else (lambda *s: torch.zeros(*s, device=dev))
    gr = dict(d_logits=mk(NS, K), d_logits_r=mk(NS, K), d_ddist=mk(NS, 2, Da), d_sdist_r=mk(NT, 2, Da))
    gr0 = {k: v.clone().cpu() for k, v in gr.items()}
    acc = torch.full((L.LOSS_SLOTS,), 3.25, dtype=torch.float64, device=dev)
    ema = d["ema"].clone()
    Pbuf = torch.full((K * K,), 7.5, device=dev)
    a = L.SmallLossArgs()
    a.K, a.Da, a.NS, a.NT = K, Da, NS, NT
    a.Pbuf, a.mi_grad_scale = Pbuf.data_ptr(), 2.0 if hook else 1.0
    a.p, a.q, a.logp = p.data_ptr(), q.data_ptr(), logp.data_ptr()
    a.ddist, a.sdist, a.sdist_r = d["ddist"].data_ptr(), d["sdist"].data_ptr(), d["sdist_r"].data_ptr()
    for n in gr:
        setattr(a, n, gr[n].data_ptr())
    a.ema, a.ema_alpha, a.update_ema = (ema.data_ptr() if use_ema else None), EMA_ALPHA, update_ema
    a.mi_lamb = lamb
    for n, v in SMALL_W.items():
        setattr(a, n, v)
    a.acc = acc.data_ptr()
    calls = []

    def double_in_place(ptr, count, user):      # in-place sum over two identical ranks, enqueued on the caller's stream
        v = TV(ptr, 1, 1, count, 1, count, 1)
        calls.append((count, lib.caddy_k_copy(C.byref(v), C.byref(v), 1, st)))
    cb = L.ALLREDUCE_HOOK(double_in_place)
    assert lib.caddy_k_loss_small(C.byref(a), cb if hook else NO_HOOK, None, st) == 0
    sync(dev)
    if hook:
        assert calls == [(K * K, 0)]
    G = "loss_small"
    accc = acc.cpu()
    for n in ("entropy", "dir_kl", "mi", "state_kl"):
        check(G, n, accc[L.LOSS_SLOT[n]], r32[n], r64[n])
    keep = torch.ones(L.LOSS_SLOTS, dtype=torch.bool)
    keep[[L.LOSS_SLOT[n] for n in ("entropy", "dir_kl", "mi", "state_kl")]] = False
    exact("other loss slots untouched", accc[keep], torch.full((L.LOSS_SLOTS - 4,), 3.25, dtype=torch.float64))
    for n in gr:
        b0 = gr0[n]
        check(G, n + (" (added to a base)" if base else ""), gr[n].cpu().double() - b0.double(), r32[n], r64[n], extra=U * b0.abs().max().item())
    exact("variance half of d_sdist_r untouched", gr["d_sdist_r"][:, 1], gr0["d_sdist_r"][:, 1])
    for n in ("sdist", "sdist_r", "ddist"):
        exact(n + " unchanged", d[n], x[n])
    if use_ema and update_ema:
        check(G, "ema (new state)", ema, r32["new_ema"], r64["new_ema"])
    else:
        exact("ema untouched", ema, x["ema"])


# ====================================================================================================================================================================================
# loss_l1: L1 between the bilinearly resized ground truth and a reconstruction
# ====================================================================================================================================================================================
def l1_case(lib, dev, *, f, t_off, B=2, Tobs=3, h=4, w=6, gt_out=False, seed=0, base=False, ties=0):
    declare(lib)
    g = torch.Generator().manual_seed(3000 + seed)
    Trec = Tobs - t_off
    gt = torch.rand(B, Tobs, 3, f * h, f * w, generator=g) * 2 - 1
    rec = torch.rand(B * Trec, 3, h, w, generator=g) * 2 - 1
    near = (F.interpolate(gt[:, t_off:].reshape(B * Trec, 3, f * h, f * w), (h, w), mode="bilinear", align_corners=False) - rec).abs() < 1e-3
    rec[near] += 4e-3      # keep the differences clear of the sign's branch point
    tie = torch.zeros(B * Trec, 3, h, w, dtype=torch.bool)
    if ties:
        assert f == 1
        idx = torch.randint(0, tie.numel(), (ties,), generator=g)
        tie.view(-1)[idx] = True
        rec = torch.where(tie, gt[:, t_off:].reshape(B * Trec, 3, h, w), rec)
    gscale = f32(0.37)

    def ref(dt):
        rr = rec.to(dt).clone().requires_grad_(True)
        gg = F.interpolate(gt[:, t_off:].reshape(B * Trec, 3, f * h, f * w).to(dt), (h, w), mode="bilinear", align_corners=False)
        s = (gg - rr).abs().sum()
        (gscale * s).backward()
        return gg.detach(), s.detach(), rr.grad
    g64, s64, d64 = ref(torch.float64)
    g32, s32, d32 = ref(torch.float32)
    assert (g64 - rec.double()).abs()[~tie].min().item() >= 1e-5, "an un-planted L1 difference below 1e-5: choose another seed"

    st = stream(dev)
    gt_d = torch.full((B * Tobs, f * h, f * w, 4), 7.5)
    gt_d[..., :3] = gt.reshape(B * Tobs, 3, f * h, f * w).permute(0, 2, 3, 1)
    rec_d = torch.full((B * Trec, h, w, 4), 7.5)
    rec_d[..., :3] = rec.permute(0, 2, 3, 1)
    gt_d, rec_d = gt_d.to(dev), rec_d.to(dev)
    drec0 = torch.randn(B * Trec, h, w, 4, generator=g) if base else torch.zeros(B * Trec, h, w, 4)
    drec = drec0.clone().to(dev)
    acc0 = 12.5 if base else 0.0
    acc = torch.full((2,), acc0, dtype=torch.float64, device=dev)
    gout = torch.full((B * Trec, h, w, 4), 7.5, device=dev) if gt_out else None
    tg = flat_tv(gt_d, B * Tobs, f * h, f * w, 3, f * h * f * w * 4, 4)
    tr, td = flat_tv(rec_d, B * Trec, h, w, 3, h * w * 4, 4), flat_tv(drec, B * Trec, h, w, 3, h * w * 4, 4)
    assert lib.caddy_k_loss_l1(C.byref(tg), C.byref(tr), C.byref(td), f, t_off, Tobs, Trec, gscale, P(acc), P(gout) if gt_out else None, st) == 0
    sync(dev)
    G = "loss_l1"
    tag = " (added to a base)" if base else ""
    check(G, "sum" + tag, acc.cpu()[0] - acc0, s32, s64, extra=U * acc0)
    exact("the neighbouring accumulator", acc.cpu()[1], torch.tensor(acc0, dtype=torch.float64))
    got = drec.cpu()
    check(G, "drec" + tag, (got[..., :3].double() - drec0[..., :3].double()).permute(0, 3, 1, 2), d32, d64, extra=U * drec0.abs().max().item())
    exact("drec pad channel untouched", got[..., 3], drec0[..., 3])
    if ties:
        exact("zero gradient at the planted ties", got[..., :3].permute(0, 3, 1, 2)[tie], drec0[..., :3].permute(0, 3, 1, 2)[tie])
    if gt_out:
        go = gout.cpu()
        check(G, "resized ground truth", go[..., :3].permute(0, 3, 1, 2), g32, g64)
        exact("gt_out pad channel untouched", go[..., 3], torch.full((B * Trec, h, w), 7.5))


# ====================================================================================================================================================================================
# loss_mse: MSE(a.detach(), b) over the first C channels, on plain tensors and on the strided views of the hidden-state loss
# ====================================================================================================================================================================================
def mse_case(lib, dev, *, N, H, W, Cc=65, ld=68, hidden_T=None, seed=0, base=False):
    """hidden_T = T: the views of HiddenStatesLoss(hidden, rec_hidden[:, 1:]) -- a: frames 1 .. T-1 of each of the N sequences of T frames, b: N sequences of T - 1 frames; each
    sequence is one image of height (T - 1) * H, so a.sn != b.sn"""
    declare(lib)
    g = torch.Generator().manual_seed(4000 + seed)
    T = hidden_T
    na, nb = (N * T, N * (T - 1)) if T else (N, N)
    A = torch.full((na, H, W, ld), 7.5); A[..., :Cc] = torch.randn(na, H, W, Cc, generator=g)
    Bt = torch.full((nb, H, W, ld), 7.5); Bt[..., :Cc] = torch.randn(nb, H, W, Cc, generator=g)
    db0 = torch.randn(nb, H, W, ld, generator=g) if base else torch.zeros(nb, H, W, ld)
    gscale = f32(0.0123)
    a_sel = A.view(N, T, H, W, ld)[:, 1:].reshape(nb, H, W, ld)[..., :Cc] if T else A[..., :Cc]

    def ref(dt):
        bb = Bt[..., :Cc].to(dt).clone().requires_grad_(True)
        s = (bb - a_sel.to(dt)).pow(2).sum()
        (gscale * s).backward()
        return s.detach(), bb.grad
    s64, d64 = ref(torch.float64)
    s32, d32 = ref(torch.float32)
    st = stream(dev)
    A_d, B_d, db = A.to(dev), Bt.to(dev), db0.clone().to(dev)
    fs = H * W * ld
    if T:
        ta = flat_tv(A_d, N, (T - 1) * H, W, Cc, T * fs, ld, off=fs)
        tb, tdb = flat_tv(B_d, N, (T - 1) * H, W, Cc, (T - 1) * fs, ld), flat_tv(db, N, (T - 1) * H, W, Cc, (T - 1) * fs, ld)
    else:
        ta, tb, tdb = flat_tv(A_d, N, H, W, Cc, fs, ld), flat_tv(B_d, N, H, W, Cc, fs, ld), flat_tv(db, N, H, W, Cc, fs, ld)
    acc0 = 12.5 if base else 0.0
    acc = torch.full((1,), acc0, dtype=torch.float64, device=dev)
    assert lib.caddy_k_loss_mse(C.byref(ta), C.byref(tb), C.byref(tdb), gscale, P(acc), st) == 0
    sync(dev)
    G = "loss_mse"
    tag = " (added to a base)" if base else ""
    check(G, "sum" + tag, acc.cpu()[0] - acc0, s32, s64, extra=U * acc0)
    got = db.cpu()
    check(G, "db" + tag, got[..., :Cc].double() - db0[..., :Cc].double(), d32, d64, extra=U * db0.abs().max().item())
    exact("db pad channels untouched", got[..., Cc:], db0[..., Cc:])
    exact("a unchanged", A_d, A)


# ====================================================================================================================================================================================
# loss_diff_per_frame: per-frame sums of the evaluation
# ====================================================================================================================================================================================
def diff_per_frame_case(lib, dev, *, Cc, ld, H, W, sq, a_off, B=2, Tb=2, seed=0):
    declare(lib)
    g = torch.Generator().manual_seed(5000 + seed)
    Ta = Tb + 1      # Ta != Tb: frame n of b meets frame (n / Tb) * Ta + n % Tb + a_off of a
    A = torch.full((B * Ta, H, W, ld), 7.5); A[..., :Cc] = torch.randn(B * Ta, H, W, Cc, generator=g)
    Bt = torch.full((B * Tb, H, W, ld), -3.5); Bt[..., :Cc] = torch.randn(B * Tb, H, W, Cc, generator=g)
    acc0 = torch.rand(B * Tb, generator=g).double() + 1.0      # the kernel adds

    def ref(dt):
        dd = A.view(B, Ta, H, W, ld)[:, a_off:a_off + Tb, ..., :Cc].to(dt) - Bt.view(B, Tb, H, W, ld)[..., :Cc].to(dt)
        return (dd.pow(2) if sq else dd.abs()).sum(dim=(2, 3, 4)).reshape(-1)
    r64, r32 = ref(torch.float64), ref(torch.float32)
    A_d, B_d, acc = A.to(dev), Bt.to(dev), acc0.clone().to(dev)
    ta, tb = flat_tv(A_d, B * Ta, H, W, Cc, H * W * ld, ld), flat_tv(B_d, B * Tb, H, W, Cc, H * W * ld, ld)
    assert lib.caddy_k_loss_diff_per_frame(C.byref(ta), Ta, a_off, C.byref(tb), Tb, Cc, sq, P(acc), stream(dev)) == 0
    sync(dev)
    check("diff_per_frame", f"sums (sq={sq}, a_off={a_off})", acc.cpu() - acc0, r32, r64, extra=U * acc0.max().item())


# ====================================================================================================================================================================================
# loss_finalize / loss_report_flag / head_softmax / loss_diagnostics
# ====================================================================================================================================================================================
def finalize_case(lib, dev, *, with_vgg, hidden=True, seed=0):
    declare(lib)
    g = torch.Generator().manual_seed(6000 + seed)
    S = L.LOSS_SLOT
    acc0 = torch.rand(L.LOSS_SLOTS, generator=g, dtype=torch.float64) * 100 + 1
    wv = (torch.rand(9, generator=g, dtype=torch.float64) + 0.1).tolist()
    n = (torch.randint(50, 5000, (5,), generator=g).double()).tolist()
    if not hidden:
        n[4] = 0.0
    numel = torch.randint(100, 100000, (3, 5), generator=g).double()

    def ref(dt):      # net.cpp's formula: means of the sums, the weighted total; trainer.py:447-466 for the perceptual levels (level 0 handed on IS the total)
        a = acc0.to(dt).clone()
        w = [torch.tensor(v, dtype=dt) for v in wv]
        nn = [torch.tensor(v, dtype=dt) for v in n]
        for r in range(3):
            a[S["l1_r0"] + r] = a[S["l1_r0"] + r] / nn[r]
        a[S["rec"]] = (a[S["l1_r0"]] + a[S["l1_r1"]] + a[S["l1_r2"]]) / 3
        a[S["states"]] = a[S["states"]] / nn[3]
        a[S["hidden"]] = a[S["hidden"]] / nn[4] if n[4] > 0 else torch.zeros((), dtype=dt)
        a[S["total"]] = (w[0] * a[S["rec"]] + w[1] * a[S["states"]] + w[2] * a[S["entropy"]] + w[3] * a[S["dir_kl"]] + w[4] * a[S["mi"]] + w[5] * a[S["state_kl"]]
                         + w[6] * a[S["hidden"]])
        if with_vgg:
            avg, term = torch.zeros((), dtype=dt), torch.zeros((), dtype=dt)
            for r in range(3):
                o = S["perc_r0"] + 6 * r
                lv = a[o + 1:o + 6] / numel[r].to(dt)
                tot, rest = lv.sum(), lv[1:].sum()
                a[o + 1:o + 6] = lv
                a[o] = tot
                a[o + 1] = tot
                avg, term = avg + tot, term + w[8] * (tot + rest)
            a[S["perceptual"]], a[S["perceptual_term"]] = avg / 3, term / 3
            a[S["total"]] = a[S["total"]] + term / 3
        return a
    r64, r32 = ref(torch.float64), ref(torch.float32)
    acc = acc0.clone().to(dev)
    lw = L.LossWeights(*wv)
    lv = L.VggLevels()
    for r in range(3):
        for l in range(5):
            lv.numel[r][l] = numel[r, l].item()
    assert lib.caddy_k_loss_finalize(P(acc), C.byref(lw), n[0], n[1], n[2], n[3], n[4], C.byref(lv) if with_vgg else None, stream(dev)) == 0
    sync(dev)
    got = acc.cpu()
    touched = {S[k] for k in ("total", "rec", "states", "hidden", "l1_r0", "l1_r1", "l1_r2")}
    if with_vgg:
        touched |= {S["perceptual"], S["perceptual_term"]} | {S["perc_r0"] + i for i in range(18)}
    for i in range(L.LOSS_SLOTS):
        if i in touched:
            check("loss_finalize", f"slot {i}", got[i], r32[i], r64[i])
        else:
            exact(f"slot {i} untouched", got[i], acc0[i])


def report_flag_case(lib, dev, n=70):
    """live and sticky halves of the f16 range-guard words: bit 0 -> slot = 1, bit 1 -> NaN total; a step's bits are reported once and moved to the sticky half"""
    declare(lib)
    st = stream(dev)
    flags = torch.zeros(2 * n, dtype=torch.int32)
    flags[3], flags[n - 1], flags[n + 5] = 1, 1, 1      # two live words (one beyond the first 64: the strided loop), one older sticky word
    want_sticky = torch.zeros(n, dtype=torch.int32)
    want_sticky[[3, n - 1, 5]] = 1
    fl = flags.to(dev)
    out = torch.tensor([5.0, 2.5], dtype=torch.float64, device=dev)      # [slot, total]

    def run():
        assert lib.caddy_k_loss_report_flag(P(fl), n, C.c_void_p(out.data_ptr()), C.c_void_p(out.data_ptr() + 8), st) == 0
        sync(dev)
        return out.cpu(), fl.cpu()
    o, f_ = run()
    assert o[0].item() == 1.0 and o[1].item() == 2.5
    exact("live half cleared", f_[:n], torch.zeros(n, dtype=torch.int32))
    exact("sticky half", f_[n:], want_sticky)
    o, f_ = run()      # reported once
    assert o[0].item() == 0.0 and o[1].item() == 2.5
    exact("sticky half kept", f_[n:], want_sticky)
    fl[n - 2] = 2      # a NaN among the clamped values, no saturation bit
    o, f_ = run()
    assert o[0].item() == 0.0 and o[1].isnan().item()
    want_sticky[n - 2] = 2
    exact("sticky half", f_[n:], want_sticky)
    out[1] = 4.0
    fl[0] = 3          # both bits
    o, f_ = run()
    assert o[0].item() == 1.0 and o[1].isnan().item()
    out[1] = 4.0
    o, f_ = run()
    assert o[0].item() == 0.0 and o[1].item() == 4.0 and f_[n].item() == 3 and f_[:n].abs().sum().item() == 0


def softmax_case(lib, dev, NS=70, K=7, seed=0):
    """head_softmax with and without the log-probabilities; one column at -200 (exact zero)"""
    declare(lib)
    g = torch.Generator().manual_seed(7000 + seed)
    lg = 2.0 * torch.randn(NS, K, generator=g)
    if K > 1:
        lg[:, K - 1] = -200.0
    lg_d = lg.to(dev)
    p1, p2, lp = (torch.full((NS, K), 7.5, device=dev) for _ in range(3))
    assert lib.caddy_k_head_softmax(P(lg_d), P(p1), None, NS, K, stream(dev)) == 0
    assert lib.caddy_k_head_softmax(P(lg_d), P(p2), P(lp), NS, K, stream(dev)) == 0
    sync(dev)
    check("head_softmax", "prob (logp null)", p1, torch.softmax(lg, 1), torch.softmax(lg.double(), 1))
    check("head_softmax", "logp", lp, torch.log_softmax(lg, 1), torch.log_softmax(lg.double(), 1))
    exact("prob with and without logp", p1, p2)
    if K > 1:
        exact("exact zeros", p1[:, K - 1], torch.zeros(NS))


DIAG_NAMES = ["samples_entropy", "action_distribution_entropy", "states_magnitude", "hidden_states_magnitude", "action_directions_mean_magnitude",
              "action_directions_variance_magnitude", "reconstructed_action_directions_mean_magnitude", "reconstructed_action_directions_variance_magnitude",
              "action_directions_reconstruction_error", "reconstructed_action_directions_kl_loss", "centroids_mean_magnitude", "average_centroids_distance",
              "average_action_variations_norm_l2", "action_variations_mean"]


def diag_case(lib, dev, *, NS, K, Da, one_hot=False, seed=0):
    """the fourteen logging scalars of the reference's loss_info (trainer.py:475-491) as playablevideogeneration_amd/trainer.py restates them"""
    declare(lib)
    g = torch.Generator().manual_seed(8000 + seed)
    r = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
    if one_hot:
        samples = F.one_hot(torch.arange(NS) % K, K).float()      # every action occurs: only slot 0 is 0 * log 0
    else:
        samples = torch.softmax(1.5 * r(NS, K), 1)
    ddist = torch.stack([r(NS, Da), 0.1 + torch.rand(NS, Da, generator=g)], 1)
    rdist = torch.stack([r(NS, Da), 0.1 + torch.rand(NS, Da, generator=g)], 1)
    var, cen = r(NS, Da), r(K, Da)
    states = torch.full((3, 5, 7, 68), 7.5); states[..., :64] = r(3, 5, 7, 64)
    hidden = torch.full((2, 9, 4, 36), 7.5); hidden[..., :33] = r(2, 9, 4, 33)

    def ref(dt):
        s, dd, rd, v, c = (a.to(dt) for a in (samples, ddist, rdist, var, cen))
        ent = lambda p: -(p * torch.log(p)).sum() / p.shape[0]      # noqa: E731   EntropyProbabilityLoss (losses.py:359-376): no epsilon
        cdist = (c.unsqueeze(0) - c.unsqueeze(1)).pow(2).sum(2).sqrt().sum() / (K * (K - 1))
        rm, rv = rd[:, 0], rd[:, 1]
        return torch.stack([ent(s), ent(s.mean(0, keepdim=True)), states[..., :64].to(dt).abs().mean(), hidden[..., :33].to(dt).abs().mean(),
                            dd[:, 0].abs().mean(), dd[:, 1].abs().mean(), rm.abs().mean(), rv.abs().mean(), (rm - dd[:, 0]).pow(2).mean(),
                            (-0.5 * (1 + torch.log(rv) - rm.pow(2) - rv).sum(1)).mean(), c.abs().mean(), cdist, v.pow(2).sum(-1).sqrt().mean(), v.mean()])
    r64, r32 = ref(torch.float64), ref(torch.float32)
    dv = [a.contiguous().to(dev) for a in (samples, ddist, rdist, var, cen)]
    st_d, hd_d = states.to(dev), hidden.to(dev)
    acc = torch.zeros(L.LOSS_SLOTS, dtype=torch.float64, device=dev)      # (slots 2 and 3 are sums that k_abs_sum adds to)
    acc[:L.LOSS_SLOT["diag_0"]] = 3.25
    da = L.DiagArgs(*[a.data_ptr() for a in dv], NS, K, Da, acc.data_ptr())
    ts, th = flat_tv(st_d, 3, 5, 7, 64, 5 * 7 * 68, 68), flat_tv(hd_d, 2, 9, 4, 33, 9 * 4 * 36, 36)
    assert lib.caddy_k_loss_diagnostics(C.byref(da), C.byref(ts), C.byref(th), stream(dev)) == 0
    sync(dev)
    got = acc.cpu()
    d0 = L.LOSS_SLOT["diag_0"]
    for i, name in enumerate(DIAG_NAMES):
        if one_hot and i == 0:
            assert r64[0].isnan().item() and r32[0].isnan().item() and got[d0].isnan().item(), "p * log p of a one-hot row is NaN in the reference formula"
        else:
            check("loss_diagnostics", name, got[d0 + i], r32[i], r64[i])
    exact("loss slots in front untouched", got[:d0], torch.full((d0,), 3.25, dtype=torch.float64))
    exact("slots behind the fourteen untouched", got[d0 + 14:], torch.zeros(L.LOSS_SLOTS - d0 - 14, dtype=torch.float64))


# parameters shared by tests/test_head_emu.py and tests/test_head_gpu.py
SMALL_EMA = ["none", "ema_kept", "ema_updated"]
MSE_CASES = [
    dict(N=2, H=3, W=5),                               # C = 65 of pitch 68
    dict(N=2, H=3, W=5, hidden_T=3, seed=1),           # the strided views of the hidden-state loss: a.sn != b.sn
    dict(N=3, H=2, W=7, hidden_T=4, seed=2, base=True),
    dict(N=2, H=3, W=5, base=True, seed=3),
    dict(N=2, H=64, W=64, seed=4),                     # 532480 items > 2048 x 256: past the block cap
]
DPF_SIZES = [dict(Cc=3, ld=4, H=8, W=8), dict(Cc=64, ld=64, H=32, W=32), dict(Cc=64, ld=64, H=64, W=64)]      # one block; 32 blocks; the 64-block cap
FINALIZE_CASES = [(False, True), (True, True), (True, False)]      # (with VggLevels, with a hidden-state count)
DIAG_CASES = [dict(NS=280, K=8, Da=8), dict(NS=3, K=3, Da=1, seed=1), dict(NS=70, K=7, Da=2, one_hot=True, seed=2)]      # NS > 256: strided rows; one-hot: slot 0 is NaN
