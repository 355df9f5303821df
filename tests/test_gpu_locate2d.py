"""GPU parity of the 2-D locators (onset_fingerprinting_amd.multilateration; csrc/ofp_locate2d.hip) against the
reference's multilateration.py run with scipy (golden g23): find_lag / find_lag_multi case for case, the
MultilateratePaired maps bit for bit, locate and locate_cc hit for hit, the batched paths row for row, the 2-D
Multilaterate and lag_intensity_map."""
import hashlib
import json

import numpy as np
import pytest
import torch

from tests.conftest import load_golden

pytestmark = pytest.mark.gpu

ROOT_TOL = 1e-6


def g23():
    return load_golden("g23_locate2d")


def rows(g, k):
    o, la, lb = g["fl/off"][k], int(g["fl/len_a"][k]), int(g["fl/len_b"][k])
    d = g["fl/data"]
    return d[o[0]:o[0] + la].astype(np.float32) / 256, d[o[1]:o[1] + lb].astype(np.float32) / 256


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def test_find_lag_every_case():
    from onset_fingerprinting_amd import multilateration as ml
    g = g23()
    for k in range(len(g["fl/lag"])):
        a, b = rows(g, k)
        assert ml.find_lag(a, b) == int(g["fl/lag"][k]), k


def test_find_lag_multi_peaks_and_order():
    from onset_fingerprinting_amd import multilateration as ml
    g = g23()
    n = len(g["fl/lag"])
    skipped = 0
    for k in range(n):
        a, b = rows(g, k)
        t, nf = int(g["fl/top_n"][k]), int(g["fl/n_found"][k])
        p, v = ml.find_lag_multi(a, b, top_n=t)
        assert p.dtype == np.int64 and v.dtype == np.float32
        want_p, want_v = g["fl/peaks"][k, :nf], g["fl/vals"][k, :nf]
        ok = len(p) == nf and np.array_equal(p, want_p)
        if ok and nf:
            ok = np.abs(v - want_v).max() <= 1e-6 * max(float(np.max(want_v)), 1e-30)
        if not ok:
            assert bool(g["fl/near_tie"][k]), (k, p, want_p, v, want_v)
            skipped += 1
    print(f"find_lag_multi: {skipped} of {n} cases skipped at a near-tie")
    assert skipped <= 0.01 * n


def test_find_lags_device_batched_equals_per_call():
    from onset_fingerprinting_amd import multilateration as ml
    g = g23()
    n = len(g["fl/lag"])
    La, Lb = int(g["fl/len_a"].max()), int(g["fl/len_b"].max())
    A = np.zeros((n, La), np.float32)
    B = np.zeros((n, Lb), np.float32)
    for k in range(n):
        a, b = rows(g, k)
        A[k, :len(a)], B[k, :len(b)] = a, b
    dev = torch.device("cuda", 0)
    lag, pl, pv, npk = ml.find_lags_device(torch.from_numpy(A).to(dev), torch.from_numpy(B).to(dev), 8,
                                           torch.from_numpy(g["fl/len_a"]).to(dev),
                                           torch.from_numpy(g["fl/len_b"]).to(dev))
    lag, pl, pv, npk = (t.cpu().numpy() for t in (lag, pl, pv, npk))
    for k in range(n):
        a, b = rows(g, k)
        assert lag[k] == ml.find_lag(a, b), k
        p, v = ml.find_lag_multi(a, b, top_n=8)
        assert npk[k] == len(p) and np.array_equal(pl[k, :len(p)], p), k
        assert np.array_equal(pv[k, :len(p)].view(np.uint32), v.view(np.uint32)), k
        assert np.isnan(pv[k, len(p):]).all()
    lag0, _, _, npk0 = ml.find_lags_device(torch.from_numpy(A).to(dev), torch.from_numpy(B).to(dev), 0,
                                           torch.from_numpy(g["fl/len_a"]).to(dev),
                                           torch.from_numpy(g["fl/len_b"]).to(dev))
    assert np.array_equal(lag0.cpu().numpy(), lag)
    assert (npk0.cpu().numpy() == 0).all()  # no peaks asked for: no slots used


def test_find_lag_non_finite_row_refused():
    from onset_fingerprinting_amd import multilateration as ml
    a = np.array([1.0, np.nan, 2.0, 0.5], np.float32)
    assert ml.find_lag(a, np.ones(3, np.float32)) == int(np.argmax(np.correlate(a, np.ones(3, np.float32), "full"))) - 3
    with pytest.raises(ValueError):
        ml.find_lag_multi(a, np.ones(3, np.float32))


def paired(name):
    from onset_fingerprinting_amd import multilateration as ml
    return ml.MultilateratePaired(**json.loads(str(g23()[f"pair/{name}/args"])))


@pytest.mark.parametrize("name", ["p4mm", "p3air", "p2"])
def test_paired_maps_bit_identical(name):
    g = g23()
    m = paired(name)
    keys = [(i, j) for i in range(len(m.sensor_locs)) for j in m.lag_maps[i]]
    assert keys == [tuple(k) for k in g[f"pair/{name}/keys"]]
    assert [sha(m.lag_maps[i][j]) for i, j in keys] == list(g[f"pair/{name}/map_sha"])
    mp = m.lag_maps[0][1]
    assert np.array_equal(np.isnan(mp), g[f"pair/{name}/map0_nan"])
    assert np.array_equal(np.nan_to_num(mp, nan=0).astype(np.int16), g[f"pair/{name}/map0"])
    assert m.res.shape == mp.shape and m.res.dtype == np.float32


@pytest.mark.parametrize("name", ["p4mm", "p3air", "p2"])
def test_paired_locate(name):
    g = g23()
    m = paired(name)
    pre = f"pair/{name}/loc"
    for k, (lags, i) in enumerate(zip(g[f"{pre}/lags"], g[f"{pre}/first"])):
        if g[f"{pre}/raised"][k]:
            with pytest.raises(TypeError):
                m.locate([int(v) for v in lags], int(i))
        else:
            r = np.array(m.locate([int(v) for v in lags], int(i)), np.float64)
            assert np.abs(r - g[f"{pre}/rphi"][k]).max() < ROOT_TOL, k
    dev = m.device
    rphi, ier = m.locate_device(torch.from_numpy(g[f"{pre}/lags"].astype(np.int32)).to(dev),
                                torch.from_numpy(g[f"{pre}/first"].astype(np.int32)).to(dev))
    ier = ier.cpu().numpy()
    assert np.array_equal(ier, g[f"{pre}/ier"])
    ok = ier == 1
    assert np.abs(rphi.cpu().numpy()[ok] - g[f"{pre}/rphi"][ok]).max() < ROOT_TOL


def cc_inputs(g, name):
    pre = f"pair/{name}/cc"
    x = g[f"{pre}/x"].astype(np.float32) / 4096
    return x, pre


@pytest.mark.parametrize("name", ["p4mm", "p3air", "p2"])
def test_paired_locate_cc(name):
    g = g23()
    m = paired(name)
    x, pre = cc_inputs(g, name)
    res_idx = list(g[f"{pre}/res_idx"])
    side = m.side
    for h in range(len(g[f"{pre}/onset"])):
        r = m.locate_cc(x, int(g[f"{pre}/onset"][h]), int(g[f"{pre}/first"][h]), left=int(g[f"{pre}/left"][h]),
                        right=int(g[f"{pre}/right"][h]))
        assert int(np.argmax(m.res)) == int(g[f"{pre}/cell"][h]), h
        assert np.array_equal(np.array(r, np.float64), g[f"{pre}/rphi"][h]), h
        if h in res_idx:
            want = g[f"{pre}/res"][res_idx.index(h)].astype(np.float32)
            assert np.array_equal(m.res.view(np.uint32), want.view(np.uint32)), h
    assert m.res.shape == (side, side)


@pytest.mark.parametrize("name", ["p4mm", "p3air", "p2"])
def test_paired_locate_cc_device_equals_per_call(name):
    g = g23()
    m = paired(name)
    x, pre = cc_inputs(g, name)
    dev = m.device
    left, right = g[f"{pre}/left"], g[f"{pre}/right"]
    for lr in sorted(set(zip(left.tolist(), right.tolist()))):  # one batch per (left, right)
        sel = np.flatnonzero((left == lr[0]) & (right == lr[1]))
        rphi, cell, status = m.locate_cc_device(torch.from_numpy(x).to(dev),
                                                torch.from_numpy(g[f"{pre}/onset"][sel]).to(dev),
                                                torch.from_numpy(g[f"{pre}/first"][sel].astype(np.int32)).to(dev),
                                                left=lr[0], right=lr[1])
        assert (status.cpu().numpy() == 0).all()
        assert np.array_equal(cell.cpu().numpy(), g[f"{pre}/cell"][sel])
        got, want = rphi.cpu().numpy(), g[f"{pre}/rphi"][sel]
        ulp = np.spacing(np.maximum(np.abs(want), 1e-300))
        assert (np.abs(got - want) <= 4 * ulp).all()


def test_paired_locate_cc_device_statuses():
    from onset_fingerprinting_amd import multilateration as ml
    m = paired("p3air")
    dev = m.device
    x = torch.zeros((2, 600, 3), dtype=torch.float32, device=dev)
    onset = torch.tensor([5, 700, 100, 100], dtype=torch.int64, device=dev)
    first = torch.tensor([0, 1, 3, 2], dtype=torch.int32, device=dev)
    clip = torch.tensor([0, 1, 0, 1], dtype=torch.int32, device=dev)
    _, cell, status = m.locate_cc_device(x, onset, first, left=10, clip=clip)
    assert status.cpu().tolist() == [ml.PAIRED_NEG_WINDOW, ml.PAIRED_EMPTY_WINDOW, ml.PAIRED_BAD_HIT, ml.PAIRED_OK]
    assert cell.cpu().tolist()[:3] == [-1, -1, -1]


def test_paired_locate_cc_groups_chain_matches_row_replay():
    from onset_fingerprinting_amd import detection
    from onset_fingerprinting_amd import multilateration as ml
    g = g23()
    m = paired("p4mm")
    x, _ = cc_inputs(g, "p4mm")
    x = x[:40000]
    xd = torch.from_numpy(np.ascontiguousarray(np.stack([x, x[::-1].copy()]))).to(m.device)
    out = detection.BatchDetector(4, 128, sr=96000).detect(xd, want_rel=False)
    groups, n_groups = detection.group_onsets_device(out, 4, max_distance=1000, min_channels=2, cap_groups=64)
    rphi, cell, status = ml.locate_cc_groups_device(xd, groups, n_groups, m)
    gr, ng = groups.cpu().numpy(), n_groups.cpu().numpy()
    rphi, cell, status = rphi.cpu().numpy(), cell.cpu().numpy(), status.cpu().numpy()
    located = 0
    for c in range(gr.shape[0]):
        for r in range(gr.shape[1]):
            if r >= ng[c]:
                assert status[c, r] == ml.PAIRED_UNUSED
                continue
            row = gr[c, r]
            present = [k for k in range(row.shape[0]) if row[k] >= 0]
            if not present:
                assert status[c, r] == ml.PAIRED_NO_CHANNEL
                continue
            i = min(present, key=lambda k: (row[k], k))
            try:
                want = m.locate_cc(xd[c].cpu().numpy(), int(row[i]), i)
            except ValueError:
                assert status[c, r] < 0
                continue
            assert status[c, r] == ml.PAIRED_OK and cell[c, r] == int(np.argmax(m.res)), (c, r)
            assert np.abs(rphi[c, r] - np.array(want)).max() <= 1e-12 * max(abs(want[1]), 1.0), (c, r)
            located += 1
    assert located >= 1


def m2d(name):
    from onset_fingerprinting_amd import multilateration as ml
    return ml.Multilaterate(**json.loads(str(g23()[f"m2d/{name}/args"])))


@pytest.mark.parametrize("name", ["m3", "m4air"])
def test_multilaterate_maps_and_legality(name):
    g = g23()
    m = m2d(name)
    S = len(m.sensor_locs)
    assert np.array_equal(np.array(m.sensor_locs, np.float64), g[f"m2d/{name}/sensor_locs"])
    for i in range(S):
        for j in range(S):
            if i == j:
                continue
            want = g[f"m2d/{name}/maps"][i, j]
            got = m.lag_maps[i][j]
            assert np.array_equal(np.isnan(got), np.isnan(want))
            assert np.array_equal(got.view(np.uint32)[~np.isnan(want)], want.view(np.uint32)[~np.isnan(want)])
            assert m.min_lags[i][j] == g[f"m2d/{name}/min"][i, j] and m.max_lags[i][j] == g[f"m2d/{name}/max"][i, j]
    assert np.array_equal(np.array(m.max_max_lags, np.float32), g[f"m2d/{name}/max_max"])
    pre = f"m2d/{name}/legal"
    for s, o, want in zip(g[f"{pre}/sensors"], g[f"{pre}/onsets"], g[f"{pre}/idx"]):
        assert m.is_legal_3d(([int(v) for v in s], [int(v) for v in o])) == (int(want[0]), int(want[1]))


@pytest.mark.parametrize("name", ["m3", "m4air"])
def test_multilaterate_locate_trace(name):
    g = g23()
    m = m2d(name)
    pre = f"m2d/{name}/trace"
    want = g[f"{pre}/res"]
    for k, (c, o) in enumerate(zip(g[f"{pre}/sensor"], g[f"{pre}/onset"])):
        r = m.locate(int(c), int(o))
        assert (r is not None) == bool(want[k, 0]), k
        if r is not None:
            assert np.abs(np.array(r, np.float64) - want[k, 1:]).max() < ROOT_TOL, k


def test_lag_intensity_map():
    from onset_fingerprinting_amd import multilateration as ml
    g = g23()
    names = sorted({k.split("/")[1] for k in g.files if k.startswith("lim/")})
    for name in names:
        kw = json.loads(str(g[f"lim/{name}/args"]))
        lag, a, b = ml.lag_intensity_map(**kw)
        assert sha(lag) == str(g[f"lim/{name}/lag_sha"]), name
        for got, key in ((a, "a"), (b, "b")):
            want = g[f"lim/{name}/{key}"]
            assert got.dtype == np.float32 and got.shape == want.shape
            assert (np.abs(got - want) <= np.spacing(np.abs(want))).all(), (name, key)
