"""numpy reference of the trainers' random stream (include/onsetfp.h, "the trainers' random stream"): Philox4x32-10,
the dropout mask and the window shifts, written from the rules alone so that the HIP code can be held to them bit for
bit."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
SITE_DROPOUT, SITE_SHIFT = 0, 1
_LO = np.uint64(0xFFFFFFFF)
_32 = np.uint64(32)


def philox4x32(counters, keys):
    """counters uint32 [n, 4], keys uint32 [n, 2] (or one key) -> uint32 [n, 4]."""
    c = np.asarray(counters, np.uint64).reshape(-1, 4).copy()
    k = np.broadcast_to(np.asarray(keys, np.uint64).reshape(-1, 2), (c.shape[0], 2)).copy()
    c0, c1, c2, c3 = c.T
    k0, k1 = k.T
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> _32) ^ c1 ^ k0, p1 & _LO, (p0 >> _32) ^ c3 ^ k1, p0 & _LO
        k0, k1 = (k0 + np.uint64(W0)) & _LO, (k1 + np.uint64(W1)) & _LO
    return np.stack([c0, c1, c2, c3], 1).astype(np.uint32)


def key_of(seed):
    assert 0 <= seed < 2 ** 64
    return np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint32)


def words(seed, epoch, site, count):
    """The first `count` words of (seed, epoch, site): word i is output i % 4 of counter (i // 4, site, epoch, 0)."""
    q = np.arange((count + 3) // 4, dtype=np.uint32)
    c = np.stack([q, np.full_like(q, site), np.full_like(q, epoch), np.zeros_like(q)], 1)
    return philox4x32(c, key_of(seed)).reshape(-1)[:count]


def threshold(p):
    assert 0.0 <= p < 1.0
    return int(p * 2 ** 32)


def scale(p):
    return np.float32(1.0 / (1.0 - p))


def dropout_mask(seed, epoch, n, F, p):
    """float32 [n, F]: 0 where dropped (word < T), float32(1 / (1 - p)) where kept."""
    w = words(seed, epoch, SITE_DROPOUT, n * F)
    return np.where(w < np.uint32(threshold(p)), np.float32(0.0), scale(p)).astype(np.float32).reshape(n, F)


def shifts(seed, epoch, n, max_shift):
    """int32 [n] in [-max_shift, max_shift]: a 32 x 32 multiply-high of the word and 2 m + 1, less m."""
    w = words(seed, epoch, SITE_SHIFT, n).astype(np.uint64)
    return ((w * np.uint64(2 * max_shift + 1)) >> _32).astype(np.int64).astype(np.int32) - np.int32(max_shift)


def shifted_windows(audio, starts, W, seed, epoch, max_shift, n_extractions):
    """audio [N, C], starts int64 [O] -> (shifts int32 [R O], windows float32 [R O, C, W]); item j = r O + i."""
    audio = np.asarray(audio, np.float32)
    starts = np.asarray(starts, np.int64)
    O = len(starts)
    sh = shifts(seed, epoch, O * n_extractions, max_shift) if max_shift else np.zeros(O * n_extractions, np.int32)
    st = np.tile(starts, n_extractions) + sh
    idx = st[:, None] + np.arange(W)[None, :]
    assert idx.min() >= 0 and idx.max() < audio.shape[0]
    return sh, np.ascontiguousarray(audio[idx].transpose(0, 2, 1))


KNOWN = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


# ---- a CPU torch replay of the trainers' recipe under this stream ---------------------------------------------------
def synthetic_hits(seed, n_onsets, channels, width, max_shift):
    """Audio [N, channels] with one hit per onset (a decaying sinusoid that reaches sensor c after a delay set by the
    hit's position), the onsets [n_onsets, channels], the start of every window and the positions y [n_onsets, 2]."""
    rng = np.random.default_rng(seed)
    gap = width + 2 * max_shift + 8
    N = gap * (n_onsets + 1)
    r, phi = np.sqrt(rng.uniform(0, 1, n_onsets)), rng.uniform(0, 2 * np.pi, n_onsets)
    pos = np.stack([r * np.cos(phi), r * np.sin(phi)], 1)
    ang = 2 * np.pi * np.arange(channels) / channels
    d = np.linalg.norm(pos[:, None, :] - np.stack([np.cos(ang), np.sin(ang)], 1)[None], axis=-1)
    delay = np.rint(d * 0.25 * width).astype(np.int64)
    onsets = (gap * (1 + np.arange(n_onsets)))[:, None] + delay
    t = np.arange(N)[None, None, :] - onsets[:, :, None]
    sig = np.where((t >= 0) & (t < width), np.exp(-np.maximum(t, 0) / (0.25 * width)) * np.sin(2 * np.pi * t / 7.0),
                   0.0) / (0.5 + d[:, :, None])
    audio = (sig.sum(0).T + rng.normal(0, 0.01, (N, channels))).astype(np.float32)
    return audio, onsets, pos.astype(np.float32)


def cnn_features(net, x):
    import torch
    return torch.flatten(net.conv_layers(x), start_dim=1)


def lcccnn_features(lnet, x):
    """The reference's CCCNN.forward up to the dropout, over the module's own torch layers."""
    import torch
    import torch.nn.functional as F
    net = lnet.model
    B, C, W = x.shape
    h = net.conv_layers(x if net.group else x.reshape(B * C, 1, W))
    V = h.shape[-1]
    f = h.reshape(B * C, -1, V)
    BC, Kc, _ = f.shape
    cc = F.conv1d(f.reshape(1, BC * Kc, V), f.reshape(BC * Kc, 1, V), groups=BC * Kc, padding=V - 1)
    return torch.flatten(F.softmax(cc.view(BC, Kc, -1).sum(dim=1), dim=-1).view(B, C, -1), start_dim=1)


def head_of(module):
    return module.model.fc if hasattr(module, "model") else module.fc


def features_of(module):
    return lcccnn_features if hasattr(module, "model") else cnn_features


def replay(module, batch_of_epoch, y, epochs, seed, p, dtype):
    """`epochs` epochs of the module's own recipe on the CPU: configure_optimizers()'s optimiser and scheduler, one full
    batch per epoch, batch_of_epoch(e) -> float32 numpy [n, C, W], the reference mask of (seed, e) multiplied in
    before fc.  -> (loss curve float64 [epochs], final parameters flat float64)."""
    import copy
    import torch
    net = copy.deepcopy(module).cpu().to(dtype).train()
    conf = net.configure_optimizers()
    opt, sched = conf["optimizer"], conf["lr_scheduler"]["scheduler"]
    feats, fc = features_of(net), head_of(net)
    yt = torch.as_tensor(y).to(dtype)
    curve = []
    for e in range(epochs):
        x = torch.from_numpy(np.ascontiguousarray(batch_of_epoch(e))).to(dtype)
        opt.zero_grad()
        h = feats(net, x)
        if p > 0:
            h = h * torch.from_numpy(dropout_mask(seed, e, h.shape[0], h.shape[1], p)).to(dtype)
        loss = module.loss(fc(h), yt)
        loss.backward()
        opt.step()
        sched.step()
        curve.append(float(loss.detach()))
    flat = torch.cat([q.detach().reshape(-1) for q in net.parameters()]).numpy().astype(np.float64)
    return np.array(curve, np.float64), flat


def one_ulp(a, k, rows=None):
    """A copy of float32 array `a` with one element (a different one for every k) moved up by one ulp; with `rows`
    (for audio [N, C]: the rows the windows read at shift 0) the element is taken from those."""
    b = np.array(a, np.float32, copy=True)
    if rows is None:
        flat = b.reshape(-1)
        i = (k * 7919 + 13) % flat.size
        flat[i] = np.nextafter(flat[i], np.float32(np.inf))
    else:
        r, c = rows[(k * 7919 + 13) % len(rows)], k % b.shape[1]
        b[r, c] = np.nextafter(b[r, c], np.float32(np.inf))
    return b


def replays(module, data, y, epochs, seed, p, source=None, n_pert=8):
    """The float32 replay, the float64 one and n_pert float32 ones with one input value moved by one ulp.  data is the
    batch x [n, C, W], or with source = (starts, W, max_shift, n_extractions) the audio [N, C], cut anew every epoch
    by the reference's shifts.  -> dict(ref32, ref64, pert [n_pert, epochs], flat [1 + n_pert, n_params])."""
    import torch

    def batches(d):
        if source is None:
            return lambda e: d
        starts, W, m, R = source
        return lambda e: shifted_windows(d, starts, W, seed, e, m, R)[1]

    c32, f32_ = replay(module, batches(data), y, epochs, seed, p, torch.float32)
    c64, _f = replay(module, batches(data), y, epochs, seed, p, torch.float64)
    rows = None if source is None else (np.asarray(source[0])[:, None] + np.arange(source[1])[None, :]).reshape(-1)
    pert = [replay(module, batches(one_ulp(data, k + 1, rows)), y, epochs, seed, p, torch.float32)
            for k in range(n_pert)]
    return dict(ref32=c32, ref64=c64, pert=np.stack([c for c, _ in pert]),
                flat=np.stack([f32_] + [f for _c, f in pert]))


def comparable_prefix(ref, pert):
    """(epochs before the disturbed curves first stray more than 1e-5 relative from ref, the spread per epoch)."""
    n = len(ref)
    with np.errstate(invalid="ignore"):
        spread = np.max(np.abs(pert[:, :n] - ref[None, :]), axis=0)
    bad = np.isnan(spread) | (spread > 1e-5 * ref)
    return (int(np.argmax(bad)) if bad.any() else n), spread
