"""CPU-only checks of the 2-D locators (onset_fingerprinting_amd.multilateration: find_lag, MultilateratePaired,
Multilaterate, lag_intensity_map): the golden g23 itself, the host helpers against the reference's results, and
argument checks that refuse before any GPU work."""
import json

import numpy as np
import pytest

from tests.conftest import load_golden


def g23():
    return load_golden("g23_locate2d")


def test_golden_shape_and_keys():
    g = g23()
    n = len(g["fl/lag"])
    assert n >= 500
    for k in ("off", "len_a", "len_b", "top_n", "n_found", "near_tie"):
        assert len(g[f"fl/{k}"]) == n, k
    assert g["fl/peaks"].shape == g["fl/vals"].shape == (n, 8)
    assert g["fl/len_a"].max() <= 4096 and g["fl/len_b"].max() <= 4096 and g["fl/len_a"].min() >= 1
    assert np.any(g["fl/len_a"] != g["fl/len_b"]) and np.any(g["fl/n_found"] < g["fl/top_n"])
    for name in ("p4mm", "p3air", "p2"):
        side = int(g[f"pair/{name}/side"])
        assert g[f"pair/{name}/map0"].shape == (side, side)
        assert g[f"pair/{name}/cc/res"].shape[1:] == (side, side)
        assert len(g[f"pair/{name}/cc/lags"]) == len(g[f"pair/{name}/cc/onset"])
    assert len(g["pair/p4mm/loc/lags"]) + len(g["pair/p3air/loc/lags"]) >= 200
    assert g["pair/p4mm/loc/raised"].any()
    assert sum(len(g[f"pair/{n}/cc/onset"]) for n in ("p4mm", "p3air", "p2")) >= 300
    assert (g["pair/p3air/cc/cell"] == 0).any()  # hits no cell matches: the corner
    assert (g["pair/p4mm/cc/left"] > 0).any()
    assert len(g["pair/p2/keys"]) == 2  # S = 2: one map per sensor
    for name in ("m3", "m4air"):
        assert len(g[f"m2d/{name}/legal/idx"]) >= 1000
    assert len([k for k in g.files if k.startswith("lim/") and k.endswith("/args")]) >= 4


def test_sensor_positions_match_reference():
    from onset_fingerprinting_amd import multilateration as ml
    g = g23()
    for name in ("p4mm", "p3air", "p2"):
        kw = json.loads(str(g[f"pair/{name}/args"]))
        radius = int(np.round(ml.DIAMETER * kw["scale"] / 2, 1))
        assert radius == int(g[f"pair/{name}/radius"])
        locs = [ml.polar_to_cartesian(r * radius, p) for r, p in kw["sensor_locations"]]
        assert np.array_equal(np.array(locs, np.float64), g[f"pair/{name}/sensor_locs"])


def test_intensity_helpers_match_reference():
    from onset_fingerprinting_amd import multilateration as ml
    g = g23()
    for name in sorted({k.split("/")[1] for k in g.files if k.startswith("lim/")}):
        kw = json.loads(str(g[f"lim/{name}/args"]))
        r = int(np.round(kw.get("d", ml.DIAMETER), 1) * kw["scale"]) // 2
        i, j = np.meshgrid(range(-r, r + 1), range(-r, r + 1))
        for mic, key in ((kw["mic_a"], "a"), (kw["mic_b"], "b")):
            a, theta = ml.attenuate_intensity((i, j, 0), np.array(mic), kw["reflectivity"],
                                              ml.sound_intensity_at_source(None))
            assert theta.shape == (i.size,)
            got = (10 * np.log10(a.reshape(i.shape))).astype(np.float32)
            assert np.array_equal(got, g[f"lim/{name}/{key}"]), (name, key)


def test_vec_sub():
    from onset_fingerprinting_amd import multilateration as ml
    v = ml.vec_sub(np.array([1.0, 2.0, 3.0]), (np.array([[0, 1]]), np.array([[2, 5]]), 1))
    assert np.array_equal(v, [[1.0, 0.0, 2.0], [0.0, -3.0, 2.0]])


def test_find_lag_refuses_before_gpu_work():
    from onset_fingerprinting_amd import multilateration as ml
    with pytest.raises(ValueError):
        ml.find_lag(np.zeros(0, np.float32), np.ones(4, np.float32))
    with pytest.raises(ValueError):
        ml.find_lag_multi(np.ones(3), np.zeros(0))
    with pytest.raises(ValueError):
        ml.find_lag(np.ones(4097), np.ones(8))
    for top_n in (-1, 17):
        with pytest.raises(ValueError):
            ml.find_lag_multi(np.ones(8), np.ones(8), top_n=top_n)


def test_paired_refuses_before_gpu_work():
    from onset_fingerprinting_amd import multilateration as ml
    with pytest.raises(ValueError):
        ml.MultilateratePaired([(0.9, 0)], scale=1)
    with pytest.raises(ValueError):
        ml.MultilateratePaired([(0.9, 20 * k) for k in range(17)], scale=1)
    m = ml.MultilateratePaired.__new__(ml.MultilateratePaired)  # the checks below run before the maps are used
    m.sensor_locs = [(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0)]
    x = np.zeros((8192, 3), np.float32)
    with pytest.raises(ValueError):
        m.locate_cc(x, 100, 0, left=0, right=4097)  # window longer than 4096
    with pytest.raises(ValueError):
        m.locate_cc(x, 10, 0, left=11)  # onset_idx - left < 0
    with pytest.raises(ValueError):
        m.locate_cc(x, 9000, 0)  # empty window
    with pytest.raises(ValueError):
        m.locate_cc(x, 100, 3)  # no such sensor
