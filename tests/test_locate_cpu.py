"""CPU-only checks of the hit locator (onset_fingerprinting_amd.multilateration): the host formulas against the
reference's (golden g22), the golden file itself, and argument checks that refuse before any GPU work."""
import json

import numpy as np
import pytest

from tests.conftest import GOLDEN, load_golden


def g22():
    return load_golden("g22_locate")


def test_speed_of_sound_matches_reference():
    from onset_fingerprinting_amd import multilateration as ml
    got = [ml.speed_of_sound(sc, t, h, md) for sc in (1, 100, 1000) for t in (0.0, 20.0, 31.5) for h in (0.0, 0.5, 0.9)
           for md in ("air", "drumhead")]
    assert np.array_equal(np.array(got, np.float64), g22()["host/speed_of_sound"])


def test_coordinate_transforms_match_reference():
    from onset_fingerprinting_amd import multilateration as ml
    g = g22()
    pts, rpt = g["host/xyz"], g["host/rpt"]
    same = lambda a, b: np.array_equal(np.array(a, np.float64), b, equal_nan=True)
    assert same([ml.cartesian_to_polar(x, y) for x, y, _ in pts], g["host/c2p"])
    assert same([ml.cartesian_to_polar(x, y, 17.78) for x, y, _ in pts], g["host/c2p_r"])
    assert same([ml.cartesian_to_spherical(x, y, z) for x, y, z in pts], g["host/c2s"])
    assert same([ml.cartesian_to_cylindrical(x, y, z, 7.0) for x, y, z in pts], g["host/c2cyl"])
    assert same([ml.polar_to_cartesian(r, p) for r, p, _ in rpt], g["host/p2c"])
    assert same([ml.spherical_to_cartesian(r, p, t) for r, p, t in rpt], g["host/s2c"])
    assert same([ml.cylindrical_to_cartesian(r, p, t) for r, p, t in rpt], g["host/cyl2c"])


def test_sensor_positions_of_the_layouts_match_reference():
    from onset_fingerprinting_amd import multilateration as ml
    g = g22()
    for name in ("rt3", "air4"):
        args = json.loads(str(g[f"m3d/{name}/args"]))
        radius = ml.DIAMETER / 2
        locs = [ml.spherical_to_cartesian(x[0] * radius, x[1], x[2]) for x in args["sensor_locations"]]
        assert np.array_equal(np.array(locs, np.float64), g[f"m3d/{name}/sensor_locs"])


def test_remove_seed():
    from onset_fingerprinting_amd import multilateration as ml
    groups = [([0, 1], [10, 20]), ([0], [10]), ([1], [10]), ([0, 2], [11, 30])]
    assert ml.remove_seed(groups, ([0, 1, 2], [10, 20, 30])) == [([1], [10]), ([0, 2], [11, 30])]


def test_golden_file_is_complete_and_consistent():
    g = g22()
    assert (GOLDEN / "g22_locate.npz").stat().st_size < 1_000_000
    for k in ("solve3", "solve2"):
        K = len(g[f"{k}/ier"])
        assert g[f"{k}/geom"].shape == (K, 9) and g[f"{k}/delta"].shape == (K, 2) and g[f"{k}/guess"].shape == (K, 2)
        assert g[f"{k}/root"].shape == (K, 2) and g[f"{k}/nfev"].shape == (K,)
        assert set(np.unique(g[f"{k}/ier"])) >= {1, 2, 5}  # converged, maxfev exhausted, no progress
    assert len(g["solve3/ier"]) >= 2000 and len(g["solve2/ier"]) >= 300
    assert np.all(g["solve2/geom"][:, 2::3] == 0)
    for name in ("rt3", "air4"):
        idx = g[f"legal/{name}/idx"]
        none = (idx[:, 0] == 0) & (idx[:, 1] == 0)
        assert len(idx) == 1000 and 0 < none.sum() < len(idx)
        S = g[f"m3d/{name}/sensor_locs"].shape[0]
        assert g[f"m3d/{name}/maps"].shape[:2] == (S, S)
        assert np.isnan(np.diagonal(g[f"m3d/{name}/min"])).all()
    shapes = {k: g[k].shape for k in g.files if k.startswith("map/") and k.endswith("/map")}
    assert (357, 357) in shapes.values() and (35, 35) in shapes.values()
    n = len(g["trace/onset"])
    assert g["trace/res_audio"].shape == (n, 3) and g["trace/res_plain"].shape == (n, 3)
    assert np.all(np.diff(g["trace/onset"]) >= 0) and np.all(g["trace/counter"] > g["trace/onset"])
    assert 0 < g["trace/res_audio"][:, 0].sum() < n
    rows = g["rows/groups"]
    assert rows.ndim == 2 and rows.shape[1] == 3 and len(g["rows/status"]) == len(rows) >= 10
    assert (g["rows/status"] == 1).sum() >= 5


def test_bad_arguments_are_refused_before_any_gpu_work():
    from onset_fingerprinting_amd import multilateration as ml
    with pytest.raises(ValueError, match="two sensors"):
        ml.lag_maps_device([[0.0, 0.0, 0.0]], 17, 8200.0, 96000, 19.0**2)
    with pytest.raises(ValueError, match="shape"):
        ml.lag_maps_device(np.zeros((3, 4)), 17, 8200.0, 96000, 19.0**2)
    with pytest.raises(ValueError, match="radius"):
        ml.lag_maps_device(np.zeros((3, 3)), -1, 8200.0, 96000, 1.0)
    with pytest.raises(ValueError, match="shape"):
        ml.solve_trilateration_3d((0, 0, 0, 0), (1, 1, 0), (2, 2, 0), 1.0, 1.0, (0.0, 0.0))
    with pytest.raises(ValueError):
        ml.solve_trilateration_3d((0, 0, 0), (1, 1, 0), (2, 2, 0), 1.0, 1.0, (0.0, 0.0, 0.0))
    with pytest.raises(ValueError):
        ml.locate_groups_device(np.zeros((1, 4, 3), np.int64), None, None)


def test_header_documents_the_locate_status_codes():
    from onset_fingerprinting_amd import multilateration as ml
    from tests.test_abi import REPO
    src = (REPO / "include" / "onsetfp.h").read_text()
    for name, value in (("UNUSED", ml.LOCATE_UNUSED), ("FEW_CHANNELS", ml.LOCATE_FEW_CHANNELS),
                        ("ILLEGAL_LAG", ml.LOCATE_ILLEGAL_LAG), ("NO_CELL", ml.LOCATE_NO_CELL)):
        assert f"#define OFP_LOCATE_{name} ({value})" in src
