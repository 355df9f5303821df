"""CPU-only checks of the planar locator's device forms (Multilaterate.locate_stream_device, locate_groups_device
with a Multilaterate, realtime.HopSession(locator=Multilaterate)): argument errors are raised before any GPU call, the
binding lists the new entry points, and the inputs tests/test_gpu_locate2d_device.py relies on hold what it needs."""
import numpy as np
import pytest

from tests import locate2d_cases as lc


def planar_stub(n_sensors=3, device=0):
    """A Multilaterate with what HopSession and locate_groups_device read before they touch the GPU."""
    import torch

    from onset_fingerprinting_amd import multilateration as ml
    m = ml.Multilaterate.__new__(ml.Multilaterate)
    m.sensor_locs = [(0.0, 0.0)] * n_sensors
    m.max_max_lags = [np.float32(324.0)] * n_sensors
    m.device = torch.device("cuda", device)
    m.sensors_dev = torch.zeros((n_sensors, 3), dtype=torch.float64)
    return m


@pytest.fixture
def no_gpu_calls(monkeypatch):
    """Any use of the library or of torch's device fails the test."""
    import torch

    from onset_fingerprinting_amd import _lib

    def refuse(*a, **k):
        raise AssertionError("a GPU call was made before the arguments were checked")

    monkeypatch.setattr(_lib, "lib", refuse)
    monkeypatch.setattr(_lib, "require_gpu", refuse)
    monkeypatch.setattr(torch.cuda, "device", refuse)


def test_new_entry_points_are_bound():
    from onset_fingerprinting_amd import _lib
    for name in ("ofp_locate_groups_2d", "ofp_locate_stream_2d", "ofp_hop_set_locator_2d"):
        assert name in _lib.SIGNATURES
    # ofp_locate_groups without its mlp argument; the hop entry as its 3-D sibling
    full, flat = _lib.SIGNATURES["ofp_locate_groups"], _lib.SIGNATURES["ofp_locate_groups_2d"]
    assert flat[0] is full[0] and len(flat[1]) == len(full[1]) - 1
    assert _lib.SIGNATURES["ofp_hop_set_locator_2d"] == _lib.SIGNATURES["ofp_hop_set_locator"]


def test_locate_groups_device_checks_its_arguments_for_a_planar_locator(no_gpu_calls):
    import torch

    from onset_fingerprinting_amd import multilateration as ml
    m = planar_stub(3)
    with pytest.raises(ValueError, match="CUDA"):  # host tensor
        ml.locate_groups_device(torch.zeros((1, 4, 3), dtype=torch.int64), None, m)
    with pytest.raises(ValueError, match="int64"):  # wrong dtype
        ml.locate_groups_device(torch.zeros((1, 4, 3), dtype=torch.int32), None, m)
    with pytest.raises(ValueError, match="int64"):  # not a tensor
        ml.locate_groups_device(np.zeros((1, 4, 3), np.int64), None, m)


def test_hop_session_checks_a_planar_locator_before_the_gpu(no_gpu_calls):
    from onset_fingerprinting_amd import realtime
    with pytest.raises(ValueError, match="sensors"):
        realtime.HopSession(4, 128, sr=96000, locator=planar_stub(3))
    with pytest.raises(ValueError, match="backtrack"):
        realtime.HopSession(3, 128, sr=96000, locator=planar_stub(3), backtrack=True)
    with pytest.raises(ValueError, match="lives on"):
        realtime.HopSession(3, 128, sr=96000, locator=planar_stub(3, device=1), device=0)
    # no section is read: a ring far too short for the 3-D locator's check passes on to the library
    with pytest.raises(AssertionError, match="GPU call"):
        realtime.HopSession(3, 128, sr=96000, n_fft=2048, ring_seconds=0.0, locator=planar_stub(3))


def test_planar_locator_struct_carries_no_audio_and_no_model():
    import torch

    from onset_fingerprinting_amd import multilateration as ml
    m = planar_stub(3)
    m.maps_dev = torch.zeros((3, 3, 3, 3), dtype=torch.float32)
    m.min_dev = m.max_dev = torch.zeros((3, 3), dtype=torch.float32)
    m.grid_radius, m.samples_per_cm, m.sr, m.radius, m.medium = 1, 11.7, 96000, 17.78, "drumhead"
    loc = m.locator_struct()
    assert (loc.use_audio, loc.max_section, loc.mlp, loc.S) == (0, 0, None, 3)
    assert loc.c == ml.speed_of_sound(100, medium="drumhead") and loc.sr == 96000.0


@pytest.mark.parametrize("name", lc.LAYOUTS)
def test_golden_traces_hold_enough_hits(name):
    sens, ons, res = lc.trace(name)
    assert len(sens) == len(ons) == len(res) and res[:, 0].sum() >= 20
    assert np.isfinite(res[res[:, 0] == 1, 1:]).all()
    # the numpy model the inputs are planned with follows the reference's trace call for call
    model = lc.HostModel(name)
    got = [model.locate(int(s), int(o)) == "located" for s, o in zip(sens, ons)]
    assert np.array_equal(got, res[:, 0] == 1)


@pytest.mark.parametrize("name", lc.LAYOUTS)
def test_group_rows_hold_every_kind_of_row(name):
    groups, n_groups = lc.group_rows(name)
    S = groups.shape[2]
    assert groups.shape == (2, lc.CAP, S) and n_groups[0] == lc.CAP and n_groups[1] < lc.CAP
    present = (groups >= 0).sum(-1)
    assert (present == 0).any() and ((present > 0) & (present < 3)).any() and (present == S - 1).any()
    ties = [r for r in groups.reshape(-1, S) if (r >= 0).sum() >= 3 and len(set(r[r >= 0])) < (r >= 0).sum()]
    assert ties
    model = lc.HostModel(name)
    reorder = 0
    for r in groups.reshape(-1, S):
        order = sorted((int(v), k) for k, v in enumerate(r) if v >= 0)[:3]
        reorder += len(order) == 3 and order[1][1] == 1 and order[2][1] != 0
    assert reorder >= 1  # second-earliest is sensor 1 and the 3-D reordering would change the geometry
    for clip in range(2):  # every outcome of the row rule occurs among the rows in use
        kinds = {lc.row_kind(model, r) for r in groups[clip, :n_groups[clip]]}
        assert kinds == {"few", "illegal", "no cell", "cell"} if clip == 0 else "cell" in kinds


def test_swapped_stream_extends_groups_by_negative_lags_and_locates():
    sens, ons = lc.swapped_stream("m3")
    assert len(sens) == len(ons) == 3 * lc.SWAPPED_ROWS
    model = lc.HostModel("m3")
    negative = located = 0
    for s, o in zip(sens, ons):
        s, o = int(s), int(o)
        # what locate is about to do: a group this sensor is not in, a negative lag that passes is_legal
        negative += any(o < g[1][0] and s not in g[0] and model.is_legal(g[0][0], s, o - g[1][0])
                        for g in model.ongoing)
        located += model.locate(s, o) == "located"
    assert negative >= 1  # a merged state machine that swapped here, as the 3-D routine does, would differ
    assert located >= 1


def test_hop_stream_locates_and_carries_onsets_that_complete_nothing():
    plan = lc.hop_plan("m3")
    assert sum(res == "located" for _, res in plan) >= 5
    assert sum(res is None for _, res in plan) >= 1
    assert len(lc.head_stream("m3")) % lc.HOP == 0
