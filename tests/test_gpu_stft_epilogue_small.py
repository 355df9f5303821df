"""The epilogue of k_stft_power (band sums, classifier tiles) with its LDS regions laid out as byte offsets from the
workgroup's shared array: power, mel and logits at frame counts that leave the 16-row tile partly filled, for a frame
inside one wave (256, 1024) and one across two (2048), on the plain mapping (3 channels) and the interleaved sliding one
(4 channels, frames of up to 1024 points), with and without the power output.

Power and mel against the fp64 references and bars of oracle/spectral_kernels.py (as tests/test_gpu_spectral_kernels.py
does, whose helpers are used); the logits against the fp64 network on the fp64 bands within the bar of
tests/test_gpu_stream.py (1e-4 of the largest logit, and relative for every logit above 1e-3 of it); the kernel with the
classifier against the kernel without it and the layer-by-layer network bit for bit; the per-hop session's bands against
the dense kernel's bits."""
import numpy as np
import pytest
import torch

import oracle
from oracle import spectral_kernels as K
from onset_fingerprinting_amd import synth
from tests.test_gpu_spectral_kernels import check_transform, guard_ok, guarded, interleave, noise_series
from tests.test_gpu_stream import RTOL, bits

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("H", [1, 15, 16, 17, 33])
@pytest.mark.parametrize("n_fft", [256, 1024, 2048])
def test_power_mel_logits_at_partly_filled_tiles(n_fft, H):
    from onset_fingerprinting_amd import data
    from onset_fingerprinting_amd.pipeline import seeded_fcnn
    hop, bins = n_fft // 4, n_fft // 2 + 1
    N = n_fft + (H - 1) * hop + 3
    mb = data.MelBank(K.MEL_SR, n_fft, 40)
    clf = seeded_fcnn(40, 8)
    mlp = clf.device_mlp(0)
    sd = {k: v.numpy() for k, v in clf.state_dict().items()}
    for n_clips, C in ((2, 3), (1, 4)):
        n_series = n_clips * C
        xs = noise_series(n_fft + 17 * H + C, n_series, N)
        x = torch.from_numpy(interleave(xs, n_clips, C)).cuda()
        runs = []  # (power, its buffer, mel, its buffer, logits, its buffer)
        for want_power in (True, False):
            P, pb = guarded(n_clips, C, H, bins) if want_power else (None, None)
            mel, mbuf = guarded(n_clips, C, H, 40)
            data.stft_power_mel_dense(x, n_fft, hop, mb, out_power=P, out_mel=mel, want_power=want_power)
            runs.append((P, pb, mel, mbuf, None, None))
            P, pb = guarded(n_clips, C, H, bins) if want_power else (None, None)
            mel, mbuf = guarded(n_clips, C, H, 40)
            log, lbuf = guarded(n_clips, C, H, 8)
            data.stft_power_mel_mlp_dense(x, n_fft, hop, mb, mlp, out_power=P, out_mel=mel, out_logits=log,
                                          want_power=want_power, want_mel=True)
            runs.append((P, pb, mel, mbuf, log, lbuf))
        log_only, lobuf = guarded(n_clips, C, H, 8)
        data.stft_power_mel_mlp_dense(x, n_fft, hop, mb, mlp, out_logits=log_only, want_power=False, want_mel=False)
        torch.cuda.synchronize()
        ctx = (n_fft, H, C)
        for r in runs:
            assert all(b is None or guard_ok(b) for b in r[1::2]), ctx
        assert guard_ok(lobuf), ctx
        # fp64 bars: every power and mel output
        check_transform("epilogue, small", xs, n_fft, hop,
                        [None if r[0] is None else r[0].cpu().numpy().reshape(n_series, H, bins) for r in runs],
                        [r[2].cpu().numpy().reshape(n_series, H, 40) for r in runs], mb.dense, ctx)
        # the same bits with and without the classifier, with and without the power output
        assert torch.equal(runs[0][0], runs[1][0]), ctx
        for r in runs[1:]:
            assert torch.equal(runs[0][2], r[2]), ctx
        chain = clf.forward_layerwise(runs[0][2].reshape(-1, 40)).reshape(n_clips, C, H, 8)
        for log in (runs[1][4], runs[3][4], log_only):
            assert np.array_equal(bits(log.cpu().numpy()), bits(chain.cpu().numpy())), ctx
        # logits against the fp64 network on the fp64 bands
        P64 = np.concatenate([oracle.dense_power_frames(xi, n_fft, hop) for xi in interleave(xs, n_clips, C)])
        ref = oracle.fcnn_forward(sd, (P64 @ mb.dense.astype(np.float64).T).reshape(-1, 40)).reshape(n_clips, C, H, 8)
        got = runs[1][4].cpu().numpy().astype(np.float64)
        scale = np.abs(ref).max()
        err = np.abs(got - ref)
        big = np.abs(ref) >= 1e-3 * scale
        print(f"\nlogits {ctx}: largest error / scale {err.max() / scale:.3g}, relative {(err[big] / np.abs(ref)[big]).max():.3g}", end="")
        assert err.max() / scale < RTOL and (err[big] / np.abs(ref)[big]).max() < RTOL, ctx


def test_hop_session_bands_equal_the_dense_kernels_bits():
    from onset_fingerprinting_amd import realtime
    from onset_fingerprinting_amd.data import MelBank, stft_power_mel_mlp_dense
    from onset_fingerprinting_amd.pipeline import seeded_fcnn
    C, B, sr, F = 2, 256, 48000, 1024
    x = synth.drum_hits(C, 0.2, sr, seed=6, period=0.05)
    nb = len(x) // B
    clf = seeded_fcnn(40, 8)
    sess = realtime.HopSession(C, B, sr=sr, n_fft=F, n_mels=40, classifier=clf)
    mel, logits = [], []
    for i in range(nb):
        r = sess(np.ascontiguousarray(x[i * B:(i + 1) * B]))
        mel.append(r["mel"])
        logits.append(r["logits"])
    sess.close()
    xp = np.concatenate([np.zeros((F - B, C), np.float32), x[: nb * B]])
    _, dmel, dlog = stft_power_mel_mlp_dense(torch.from_numpy(xp).cuda()[None], F, B, MelBank(sr, F, 40), clf.device_mlp(0))
    assert nb > 30 and dmel.shape[2] == nb
    assert np.array_equal(bits(dmel[0].cpu().numpy()), bits(np.stack(mel, axis=1)))
    assert np.array_equal(bits(dlog[0].cpu().numpy()), bits(np.stack(logits, axis=1)))
