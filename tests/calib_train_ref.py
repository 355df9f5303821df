"""float64 references of the two calibration kernels (csrc/ofp_train.hip): the position fit's loss and gradients
(k_tdoa_fit), the whole position fit restated over torch's own optimiser, and the BatchNorm running statistics of the
FCNN trainer (k_fcnn_train).  Written from the formulas; every result is a (value, bound) pair, the bound derived
from the roundings a float32 kernel has to make, not from what the kernels give.  u = 2^-24 is the unit roundoff of
float32 (taken 1 / 1000 larger, which covers the second-order terms the derivations drop).

Also here: float32 emulations of the kernels' expressions with planted faults (emu_*(..., fault=)), which
tests/test_calib_train_ref_cpu.py uses to show that the bounds accept a correct kernel and reject a wrong one, and
the inputs both test files share.

The position fit, per sound n with sensors s_i (pairs 0-2 and 1-3), N sounds:
    d_i = |p_n - s_i|,  t_k = (d_k - d_{k+2}) / c,  r_k = t_k - obs_k            k = 0, 1
    loss = mean |r| (L1) or mean r^2 (MSE) over the 2 N residuals;  dl_k = sign(r_k) / 2N  or  2 r_k / 2N
    d loss / d c   = -sum_n sum_k dl_k t_k / c
    d loss / d s_i = -sum_n g_i (p_n - s_i) / d_i,   g = (dl_0, dl_1, -dl_0, -dl_1) / c
    d loss / d p_n =  sum_i g_i (p_n - s_i) / d_i    (x and y only)
Reduction shape of the summed outputs (csrc/ofp_train.hip): thread tid adds the terms of sounds tid, tid + 256, ...
in ascending order (ceil(N / 256) additions), a 6-step xor butterfly joins a wave's 64 lanes, 3 additions join the
four waves: every term passes through at most D = ceil(N / 256) + 9 rounded additions, and the roundings of one
level add up to at most u sum |terms|, so the summation loses at most D u sum |terms|."""
import copy
import math

import numpy as np
import torch
from torch import nn

U = 2.0 ** -24 * 1.001
f32, f64 = np.float32, np.float64
KT = 256
RADIUS = 0.1778
LOSSES = {"l1": 0, "mse": 1}
TDOA_FAULTS = ("drop_largest", "drop_256", "lags0", "sign0", "mse_half")
STATS_FAULTS = ("biased_var", "momenta_swapped")


def sum_depth(n):
    return -(-n // KT) + 9


# ---- inputs ----------------------------------------------------------------------------------------------------

def nominal_sensors():
    """Four sensors at 0.9 of the radius on the axes, z = 0, exactly symmetric."""
    a = f32(0.9 * RADIUS)
    return np.array([[a, 0, 0], [0, a, 0], [-a, 0, 0], [0, -a, 0]], f32)


def tdoa_times64(sensors, sounds_xy, c):
    s, p = sensors.astype(f64), sounds_xy.astype(f64)
    d = np.sqrt((p[:, None, 0] - s[None, :, 0]) ** 2 + (p[:, None, 1] - s[None, :, 1]) ** 2 + s[None, :, 2] ** 2)
    return (d[:, :2] - d[:, 2:]) / float(c), d


def make_tdoa_inputs(n, seed, zero_case=False):
    """(obs [n, 2] seconds, sensors [4, 3], sounds [n, 2], c), all float32.  Hits inside the drum, starts disturbed
    by a few millimetres.  The observed times are made, not sampled: obs = float32(t64(start) +- v), v uniform in
    [2e-6, 2e-5] s, so that every float64 residual at the start is at least 1e-6 s (the rounding of t is below
    1e-9 s) and no L1 sign is in doubt.  zero_case: symmetric sensors, sound 0 at the origin with obs = 0, so that
    both of its residuals are exactly 0 in any precision."""
    rng = np.random.default_rng(seed)
    sensors = nominal_sensors()
    if not zero_case:
        sensors = (sensors.astype(f64) + rng.normal(0, 0.003, (4, 3))).astype(f32)
    r = RADIUS * np.sqrt(rng.uniform(0, 1, n))
    phi = rng.uniform(0, 2 * np.pi, n)
    sounds = (np.stack([r * np.cos(phi), r * np.sin(phi)], 1) + rng.normal(0, 0.003, (n, 2))).astype(f32)
    c = f32(335.0 + rng.uniform(0, 10))
    if zero_case:
        sounds[0] = 0.0
    t, _d = tdoa_times64(sensors, sounds, c)
    v = rng.uniform(2e-6, 2e-5, (n, 2)) * rng.choice([-1.0, 1.0], (n, 2))
    obs = (t + v).astype(f32)
    if zero_case:
        obs[0] = 0.0
    return obs, sensors, sounds, c


def residual_margin(obs, sensors, sounds_xy, c):
    """Smallest |r| of the float64 residuals that are not exactly 0."""
    t, _d = tdoa_times64(sensors, sounds_xy, c)
    r = np.abs(t - obs.astype(f64))
    return float(r[r > 0].min())


# ---- the position fit's loss and gradients, float64 with bounds -------------------------------------------------

def tdoa_loss_and_grads_ref(obs, sensors, sounds_xy, c, loss):
    """obs [N, 2] s, sensors [4, 3], sounds_xy [N, 2], c; loss "l1" or "mse".
    -> {"loss", "sensors" [4, 3], "sounds" [N, 2], "C"}: (value, bound), and "terms": the float64 per-sound terms
    of the summed outputs ({"loss" [N], "sensors" [N, 4, 3], "C" [N]}, signed as they enter the sum).

    Roundings of the float32 evaluation, per sound (all relative errors in units of u):
      p - s_i        1 per component;  d_i: squares 3, two additions 5, the root halves and adds 1: 3.5
      t_k            |dt| <= e_t = (3.5 (d_a + d_b) + 2 |d_a - d_b|) u / c    (scales with d_a + d_b, not with |t|)
      r_k            |dr| <= e_t + u |r|
      dl_k           L1: the constant 1 / 2N, 1;  MSE: (2 / 2N) dr + 2 u |dl|
      loss term      L1: |r_0| + |r_1|: dr_0 + dr_1 + u term;  MSE: 2 |r| dr + dr^2 + u r^2 each, + u term
      C term         p_k = dl_k t_k / c: |ddl| |t| / c + |dl| e_t / c + 2 u |p_k|; the term -p_0 - p_1: + u
      g_i = dl / c   ddl / c + u |g|;  f = g / (2 d): + 4.5 u;  f (2 (p - s)): + 2 u   -> 7.5 u and ddl's share
      sound term     sum of four in order: + 3 u sum |.|
    and D u sum |terms| for every summed output; the loss's factor 1 / 2N adds 2 u."""
    assert loss in LOSSES
    o, s, p, c = obs.astype(f64), sensors.astype(f64), sounds_xy.astype(f64), float(c)
    N = len(p)
    D = sum_depth(N)
    df = np.stack([p[:, None, 0] - s[None, :, 0], p[:, None, 1] - s[None, :, 1],
                   np.broadcast_to(-s[None, :, 2], (N, 4))], 2)            # [N, 4, 3]
    d = np.sqrt((df ** 2).sum(2))                                          # [N, 4]
    t = (d[:, :2] - d[:, 2:]) / c                                          # [N, 2]
    e_t = (3.5 * (d[:, :2] + d[:, 2:]) + 2 * np.abs(d[:, :2] - d[:, 2:])) * U / c
    r = t - o
    dr = e_t + U * np.abs(r)
    if loss == "l1":
        lterm = np.abs(r).sum(1)
        b_lterm = dr.sum(1) + U * lterm
        dl = np.sign(r) / (2 * N)
        ddl = U * np.abs(dl)
    else:
        lterm = (r ** 2).sum(1)
        b_lterm = (2 * np.abs(r) * dr + dr ** 2 + U * r ** 2).sum(1) + U * lterm
        dl = 2 * r / (2 * N)
        ddl = dr / N + 2 * U * np.abs(dl)
    val = lterm.sum() / (2 * N)
    b_loss = (b_lterm.sum() + D * U * lterm.sum()) / (2 * N) + 2 * U * val

    pk = dl * t / c
    b_pk = ddl * np.abs(t) / c + np.abs(dl) * e_t / c + 2 * U * np.abs(pk)
    cterm = -pk.sum(1)
    b_cterm = b_pk.sum(1) + U * np.abs(pk).sum(1)
    g_c = cterm.sum()
    b_c = b_cterm.sum() + D * U * np.abs(pk).sum()

    g = np.concatenate([dl, -dl], 1) / c                                   # [N, 4]
    dg = np.concatenate([ddl, ddl], 1) / c + U * np.abs(g)
    fx = g[:, :, None] * df / d[:, :, None]                                # [N, 4, 3]
    b_fx = np.abs(df) / d[:, :, None] * dg[:, :, None] + 6.5 * U * np.abs(fx)
    g_sens = -fx.sum(0)
    b_sens = b_fx.sum(0) + D * U * np.abs(fx).sum(0)
    g_snd = fx[:, :, :2].sum(1)
    b_snd = b_fx[:, :, :2].sum(1) + 3 * U * np.abs(fx[:, :, :2]).sum(1)
    return {"loss": (val, b_loss), "sensors": (g_sens, b_sens), "sounds": (g_snd, b_snd), "C": (g_c, b_c),
            "terms": {"loss": lterm, "sensors": -fx, "C": cterm}}


# ---- float32 emulation of k_tdoa_fit's first epoch --------------------------------------------------------------

def sum_ascending(terms):
    """float32 sum over axis 0 in ascending order."""
    acc = np.zeros(terms.shape[1:], f32)
    for row in terms.astype(f32):
        acc = acc + row
    return acc


def sum_tree(terms):
    """float32 sum over axis 0 in the kernel's order: per-thread strided chains, butterfly per wave, waves in order."""
    t = terms.astype(f32)
    n = len(t)
    passes = -(-n // KT)
    pad = np.zeros((passes * KT,) + t.shape[1:], f32)
    pad[:n] = t
    pad = pad.reshape((passes, KT) + t.shape[1:])
    acc = np.zeros((KT,) + t.shape[1:], f32)
    for k in range(passes):
        acc = acc + pad[k]
    v = acc.reshape((KT // 64, 64) + t.shape[1:])
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lanes ^ off]
    w = v[:, 0]
    return ((w[0] + w[1]) + w[2]) + w[3]


def emu_tdoa_loss_and_grads(obs, sensors, sounds_xy, c, loss, order="tree", fault=None):
    """The kernel's float32 expressions, operation by operation, for one problem.  fault: None, "drop_largest" (every
    summed output loses the sound with its largest term), "drop_256" (sounds 256.. are missing from the sums),
    "sign0" (sign(0) = +1), "mse_half" (MSE scale 1 / numel).  "terms" [N, 14]: what every sound adds to the 12
    sensor sums, C's and the loss's."""
    assert fault in (None,) + TDOA_FAULTS and order in ("tree", "ascending")
    o, s, p, c = obs.astype(f32), sensors.astype(f32), sounds_xy.astype(f32), f32(c)
    N = len(p)
    zero, one, two = f32(0), f32(1), f32(2)
    inv_numel = one / f32(2 * N)
    mse_scale = two / f32(2 * N)
    if fault == "mse_half":
        mse_scale = inv_numel
    x, y = p[:, 0], p[:, 1]
    df = [(x - s[i, 0], y - s[i, 1], np.full(N, zero - s[i, 2], f32)) for i in range(4)]
    dist = [np.sqrt((a * a + b * b) + z * z) for a, b, z in df]
    t0, t1 = (dist[0] - dist[2]) / c, (dist[1] - dist[3]) / c
    r0, r1 = t0 - o[:, 0], t1 - o[:, 1]
    if loss == "l1":
        lterm = np.abs(r0) + np.abs(r1)
        at0 = inv_numel if fault == "sign0" else zero
        dl0 = np.where(r0 > 0, inv_numel, np.where(r0 < 0, -inv_numel, at0)).astype(f32)
        dl1 = np.where(r1 > 0, inv_numel, np.where(r1 < 0, -inv_numel, at0)).astype(f32)
    else:
        lterm = r0 * r0 + r1 * r1
        dl0, dl1 = mse_scale * r0, mse_scale * r1
    cterm = -(dl0 * (t0 / c)) - (dl1 * (t1 / c))
    gd = [dl0 / c, dl1 / c, -(dl0 / c), -(dl1 / c)]
    gx, gy = np.zeros(N, f32), np.zeros(N, f32)
    sterm = np.zeros((N, 12), f32)
    for i in range(4):
        f = gd[i] / (two * dist[i])
        fx, fy, fz = f * (two * df[i][0]), f * (two * df[i][1]), f * (two * df[i][2])
        gx, gy = gx + fx, gy + fy
        sterm[:, 3 * i], sterm[:, 3 * i + 1], sterm[:, 3 * i + 2] = -fx, -fy, -fz
    terms = np.concatenate([sterm, cterm[:, None], lterm[:, None]], 1).astype(f32)   # acc[0..13]
    if fault == "drop_largest":
        terms = terms.copy()
        for k in range(terms.shape[1]):
            terms[np.argmax(np.abs(terms[:, k])), k] = 0
    if fault == "drop_256":
        terms = terms[:KT]
    acc = (sum_tree if order == "tree" else sum_ascending)(terms)
    assert acc.dtype == f32 and gx.dtype == f32
    return {"loss": acc[13] * inv_numel, "sensors": acc[:12].reshape(4, 3), "sounds": np.stack([gx, gy], 1),
            "C": acc[12], "terms": terms}


def emu_tdoa_batch(obs, sensors, sounds_xy, c, loss, order="tree", fault=None):
    """M problems with their own lags obs [M, N, 2]; fault "lags0": every problem reads problem 0's lags."""
    out = []
    for m in range(len(sensors)):
        om = obs[0] if fault == "lags0" else obs[m]
        out.append(emu_tdoa_loss_and_grads(om, sensors[m], sounds_xy[m], c[m], loss, order,
                                           None if fault == "lags0" else fault))
    return out


def worst_ratio(got, ref, keys=("loss", "sensors", "sounds", "C")):
    """{key: max |got - value| / bound} (0 / 0 counts as 0, x / 0 as inf)."""
    out = {}
    for k in keys:
        val, bound = ref[k]
        err = np.abs(np.asarray(got[k], f64) - val)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err == 0, 0.0, err / bound)
        out[k] = float(np.max(ratio))
    return out


# ---- the whole position fit over torch's own optimiser ----------------------------------------------------------

def tdoa_fit_ref(lags, sensors0, sounds0, lr=0.01, loss="mse", num_epochs=1000, C=342.29, sr=96000, eps=1e-12,
                 patience=10, dtype=torch.float32):
    """optimize_positions restated: the four sensors, x and y of every sound and the speed of sound are fitted to
    the observed times lags / sr by full-batch Adam (one group each, learning rates lr x (2e-3, 1e-4, 0.1) held in
    float32), cosine annealing over num_epochs, and gradients clipped to norm 1.  Before every update the loss is
    compared with the best so far: a loss that is not below best - eps uses up one unit of patience, and once none
    is left the loop ends without recording that loss or updating.  In float64 the inputs are the float32 values
    the kernel receives.
    -> {"curve": every loss evaluated (the stopping epoch's included), "updates", "stop_loss" (None when the loop
        ran out), "sensors" [4, 3], "sounds" [N, 3] (the positions the last forward pass used), "C", "history":
        per evaluated loss the (sensors, sounds xy, C) it was evaluated at}"""
    assert loss in LOSSES
    lossfun = nn.functional.l1_loss if loss == "l1" else nn.functional.mse_loss
    obs = (torch.as_tensor(lags, dtype=torch.float32) / sr).to(dtype)
    start = lambda v: torch.as_tensor(v, dtype=torch.float32).to(dtype).clone().requires_grad_(True)
    c = start(C)
    sens = start(np.asarray(sensors0))
    xy = start(np.asarray(sounds0)[:, :2])
    zeros = torch.zeros(len(xy), 1, dtype=dtype)
    lrs = torch.tensor([2e-3, 1e-4, 0.1], dtype=torch.float32) * lr
    rate = (lambda k: lrs[k]) if dtype == torch.float32 else (lambda k: float(lrs[k]))
    opt = torch.optim.Adam([{"params": [sens], "lr": rate(0)}, {"params": [xy], "lr": rate(1)},
                            {"params": [c], "lr": rate(2)}])
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, num_epochs)
    curve, history = [], []
    best, used, updates, stop_loss = math.inf, 0, 0, None
    used_xyz = None
    for _epoch in range(num_epochs):
        opt.zero_grad()
        used_xyz = torch.cat((xy, zeros), 1)
        dist = (used_xyz[:, None, :] - sens[None, :, :]).pow(2).sum(-1).sqrt()
        v = lossfun((dist[:, :2] - dist[:, 2:]) / c, obs)
        curve.append(float(v.detach()))
        history.append((sens.detach().numpy().copy(), xy.detach().numpy().copy(), float(c.detach())))
        if v < best - eps:
            best, used = v.detach(), 0
        elif used < patience:
            used += 1
        else:
            stop_loss = float(v.detach())
            break
        v.backward()
        torch.nn.utils.clip_grad_norm_([sens, xy, c], 1)
        opt.step()
        sched.step()
        updates += 1
    return {"curve": np.array(curve, f64), "updates": updates, "stop_loss": stop_loss,
            "sensors": sens.detach().numpy().astype(f64), "sounds": used_xyz.detach().numpy().astype(f64),
            "C": float(c.detach()), "history": history}


def short_fit_bounds(ref64, ref32, pert32, floors):
    """The short-fit rule per output: max(4 x max(spread, |ref32 - ref64|), floor), spread = the largest distance of
    the disturbed float32 runs from the undisturbed one.  -> {key: bound array}"""
    out = {}
    for k, floor in floors.items():
        a64, a32 = np.asarray(ref64[k], f64), np.asarray(ref32[k], f64)
        spread = np.max([np.abs(np.asarray(p[k], f64) - a32) for p in pert32], axis=0)
        out[k] = np.maximum(4 * np.maximum(spread, np.abs(a32 - a64)), floor)
    return out


def tdoa_short_fit_case(inputs, loss, num_epochs, eps=1e-12, patience=10, lr=0.01):
    """ref64, and the bounds of the short-fit rule for "curve", "sensors", "sounds", "C": the float32 runs are the
    restated loop on the inputs and on the lags scaled by 1 + k 2^-23, k = 1..8.  The loss's floor is its derived
    bound at the point the float64 run evaluated it, a parameter's 2^-23 x max |ref64|."""
    obs, sensors, sounds, c = inputs
    run = lambda o, dt: tdoa_fit_ref(o, sensors, sounds, lr, loss, num_epochs, float(c), 1, eps, patience, dt)
    ref64, ref32 = run(obs, torch.float64), run(obs, torch.float32)
    pert = [run(obs * f32(1 + k * 2.0 ** -23), torch.float32) for k in range(1, 9)]
    assert all(len(p["curve"]) == len(ref64["curve"]) for p in pert + [ref32])
    floor_loss = np.array([tdoa_loss_and_grads_ref(obs, s.astype(f32), p.astype(f32), f32(cc), loss)["loss"][1]
                           for s, p, cc in ref64["history"]])
    floors = {"curve": floor_loss}
    for k in ("sensors", "sounds", "C"):
        floors[k] = 2.0 ** -23 * np.max(np.abs(ref64[k]))
    return ref64, short_fit_bounds(ref64, ref32, pert, floors)


# ---- BatchNorm running statistics of the FCNN trainer -----------------------------------------------------------

ACT_LIPSCHITZ = {"Identity": 1.0, "ReLU": 1.0, "SiLU": 1.1, "LeakyReLU": 1.0, "ELU": 1.0, "Tanh": 1.0}


def _act64(name, y):
    if name == "Identity":
        return y
    if name == "ReLU":
        return np.maximum(y, 0)
    if name == "SiLU":
        return y / (1 + np.exp(-y))
    if name == "LeakyReLU":
        return np.where(y >= 0, y, 0.01 * y)
    if name == "ELU":
        return np.where(y > 0, y, np.expm1(np.minimum(y, 0)))
    assert name == "Tanh"
    return np.tanh(y)


def fcnn_layers(network):
    """[(weight, bias or None, BatchNorm1d or None, activation name)] of the hidden layers of an FCNN's Sequential."""
    mods = list(network)
    out, i = [], 0
    while i < len(mods):
        lin = mods[i]
        assert isinstance(lin, nn.Linear)
        i += 1
        bn = None
        if i < len(mods) and isinstance(mods[i], nn.BatchNorm1d):
            bn, i = mods[i], i + 1
        if i < len(mods) and not isinstance(mods[i], nn.Linear):
            out.append((lin, bn, type(mods[i]).__name__))
            i += 1
    return out


def train_fcnn_torch(network, x, y, lr, loss, num_epochs, dtype, eps=1e-9, patience=10):
    """The location-model training loop restated over torch's own modules on a copy of `network` in `dtype`:
    full-batch Adam, cosine annealing with T_max = num_epochs / 10, gradients clipped to norm 1; the early stop
    as in tdoa_fit_ref, but the loss is recorded first.  -> the trained copy (training mode)."""
    lossfun = nn.functional.l1_loss if loss == "l1" else nn.functional.mse_loss
    net = copy.deepcopy(network).to(dtype).train()
    xd, yd = torch.as_tensor(x, dtype=torch.float32).to(dtype), torch.as_tensor(y, dtype=torch.float32).to(dtype)
    opt = torch.optim.Adam([{"params": net.parameters(), "lr": lr}])
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, num_epochs / 10)
    best, used = math.inf, 0
    for _epoch in range(num_epochs):
        opt.zero_grad(set_to_none=True)
        v = lossfun(net(xd), yd)
        if v < best - eps:
            best, used = v.detach(), 0
        elif used < patience:
            used += 1
        else:
            break
        v.backward()
        torch.nn.utils.clip_grad_norm_(net.parameters(), 1)
        opt.step()
        sched.step()
    return net


def running_stats_of(network):
    return [(m.running_mean.detach().numpy().astype(f64), m.running_var.detach().numpy().astype(f64))
            for m in network if isinstance(m, nn.BatchNorm1d)]


def fcnn_running_stats_ref(network, x, y=None, lr=0.01, loss="l1", num_epochs=1):
    """BatchNorm running mean and variance, [(mean, var)] per BatchNorm layer, after num_epochs epochs of the FCNN
    trainer in float64: running <- 0.1 batch + 0.9 running, the variance from the unbiased q / (N - 1).
    num_epochs = 1 needs no optimiser step (the statistics are updated in the forward pass, with the starting
    parameters) and is evaluated here from the formulas, every entry a (value, bound) pair; more epochs train a
    float64 copy of the torch modules and give values only.

    Bounds for one epoch, carried from layer to layer (eA: error of the layer's input activations, 0 for x):
      z      a float32 dot product of `in` terms from the bias: sum_k |w_k| eA_k + (in + 1) u (sum_k |a_k w_k| + |b|)
      mean   compensated float32 sums per lane (2 u), up to 6 plain additions joining the lanes, the division:
             avg dz + 9 u avg |z|
      q      dd = z - mean: dz + dmean + u |dd|;  dd^2: 2 |dd| ddd + ddd^2 + u dd^2;  summed as the mean: 8 u more
      var    biased q / N for the normalisation, q / (N - 1) for the running variance: one division each
      running  0.1f and 0.9f are float32 constants (1 each), two products, one addition: 4 u (|0.1 new| +
             |0.9 old|), plus 0.1 of the new value's error
      y      (z - mean) invstd gamma + beta, invstd = 1 / sqrt(var + 1e-5f) (the sum 2, root and reciprocal 2)
      act    Lipschitz constant x dy + 8 u |a| (the device's expf, expm1f, tanhf are good to a few ulp)"""
    layers = fcnn_layers(network)
    assert any(bn is not None for _l, bn, _a in layers)
    if num_epochs > 1:
        return running_stats_of(train_fcnn_torch(network, x, y, lr, loss, num_epochs, torch.float64))
    a = np.asarray(x, f32).astype(f64)
    N = len(a)
    eA = np.zeros_like(a)
    out = []
    for lin, bn, act in layers:
        W = lin.weight.detach().numpy().astype(f64)
        b = lin.bias.detach().numpy().astype(f64) if lin.bias is not None else np.zeros(len(W))
        fin = W.shape[1]
        z = a @ W.T + b
        dz = eA @ np.abs(W).T + (fin + 1) * U * (np.abs(a) @ np.abs(W).T + np.abs(b))
        mean = z.mean(0)
        dmean = dz.mean(0) + 9 * U * np.abs(z).mean(0)
        dd = z - mean
        ddd = dz + dmean + U * np.abs(dd)
        q = (dd ** 2).sum(0)
        dq = (2 * np.abs(dd) * ddd + ddd ** 2).sum(0) + 9 * U * q
        unbiased = q / (N - 1)
        dunb = dq / (N - 1) + U * unbiased
        rm0 = bn.running_mean.detach().numpy().astype(f64)
        rv0 = bn.running_var.detach().numpy().astype(f64)
        rm, rv = 0.1 * mean + 0.9 * rm0, 0.1 * unbiased + 0.9 * rv0
        b_rm = 4 * U * (np.abs(0.1 * mean) + np.abs(0.9 * rm0)) + 0.1 * dmean
        b_rv = 4 * U * (np.abs(0.1 * unbiased) + np.abs(0.9 * rv0)) + 0.1 * dunb
        out.append(((rm, b_rm), (rv, b_rv)))
        var = q / N
        dvar = dq / N + U * var
        invstd = 1 / np.sqrt(var + 1e-5)
        dinv = invstd * (0.5 * (dvar + 2 * U * (var + 1e-5)) / (var + 1e-5) + 2 * U)
        ga, be = bn.weight.detach().numpy().astype(f64), bn.bias.detach().numpy().astype(f64)
        yv = dd * invstd * ga + be
        dy = np.abs(invstd * ga) * ddd + np.abs(dd * ga) * dinv + 2 * U * np.abs(dd * invstd * ga) + U * np.abs(yv)
        a = _act64(act, yv)
        eA = ACT_LIPSCHITZ[act] * dy + 8 * U * np.abs(a)
    return out


def emu_fcnn_running_stats(network, x, fault=None):
    """float32 emulation of the trainer's first forward pass (sums in ascending order, float32 throughout);
    fault: None, "biased_var" (running variance from q / N), "momenta_swapped" (0.9 batch + 0.1 running)."""
    assert fault in (None,) + STATS_FAULTS
    a = np.asarray(x, f32)
    N = len(a)
    m_new, m_old = (f32(0.9), f32(0.1)) if fault == "momenta_swapped" else (f32(0.1), f32(0.9))
    out = []
    for lin, bn, act in fcnn_layers(network):
        W = lin.weight.detach().numpy().astype(f32)
        z = np.zeros((N, len(W)), f32) + (lin.bias.detach().numpy().astype(f32) if lin.bias is not None else f32(0))
        for k in range(W.shape[1]):
            z = (a[:, k:k + 1].astype(f64) * W[None, :, k].astype(f64) + z.astype(f64)).astype(f32)   # fmaf
        mean = sum_ascending(z) / f32(N)
        dd = z - mean
        q = sum_ascending(dd * dd)
        spread = q / f32(N if fault == "biased_var" else N - 1)
        rm0, rv0 = bn.running_mean.detach().numpy().astype(f32), bn.running_var.detach().numpy().astype(f32)
        out.append((m_new * mean + m_old * rm0, m_new * spread + m_old * rv0))
        invstd = f32(1) / np.sqrt(q / f32(N) + f32(1e-5))
        yv = dd * invstd * bn.weight.detach().numpy().astype(f32) + bn.bias.detach().numpy().astype(f32)
        a = _act64(act, yv.astype(f64)).astype(f32)
        assert a.dtype == f32 and out[-1][1].dtype == f32
    return out
