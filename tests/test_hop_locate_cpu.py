"""CPU-only checks of the locator inside the hop (realtime.HopSession(locator=...)): argument errors are raised
before any GPU call, and the committed fixture g25 holds what its generator promises."""
import json
import types

import numpy as np
import pytest

from tests.conftest import load_golden


def stub(n_sensors=3, max_lag=324.0, model=None, device=0):
    """What HopSession reads of a Multilaterate3D before it touches the GPU."""
    import torch
    return types.SimpleNamespace(sensor_locs=[(0.0, 0.0, 0.0)] * n_sensors,
                                 max_max_lags=[np.float32(max_lag)] * n_sensors, model=model,
                                 device=torch.device("cuda", device))


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


def test_sensor_count_must_match(no_gpu_calls):
    from onset_fingerprinting_amd import realtime
    with pytest.raises(ValueError, match="sensors"):
        realtime.HopSession(4, 128, sr=96000, locator=stub(3))


def test_backtrack_is_refused(no_gpu_calls):
    from onset_fingerprinting_amd import realtime
    with pytest.raises(ValueError, match="backtrack"):
        realtime.HopSession(3, 128, sr=96000, locator=stub(3), backtrack=True)


def test_ring_must_hold_the_longest_section(no_gpu_calls):
    from onset_fingerprinting_amd import multilateration as ml
    from onset_fingerprinting_amd import realtime
    need = ml.longest_section(stub(3, 3000.0).max_max_lags, 128)
    assert need == 3000 + 128 + ml.lookaround + 1
    with pytest.raises(ValueError, match="ring"):  # 2048 rows (n_fft) < the section of a 3000-sample lag
        realtime.HopSession(3, 128, sr=96000, n_fft=2048, ring_seconds=0.0, locator=stub(3, 3000.0))
    with pytest.raises(ValueError, match="ring"):  # longer than the state machine's bound, whatever the ring
        realtime.HopSession(3, 128, sr=96000, locator=stub(3, 5000.0))


def test_model_must_be_a_2_to_2_fcnn(no_gpu_calls):
    import torch

    from onset_fingerprinting_amd import calibration, realtime
    with pytest.raises(ValueError, match="FCNN"):
        realtime.HopSession(3, 128, sr=96000, locator=stub(3, model=torch.nn.Linear(2, 2)))
    with pytest.raises(ValueError, match="2 -> 2"):
        realtime.HopSession(3, 128, sr=96000, locator=stub(3, model=calibration.FCNN(3, 2, hidden_layers=[4])))
    with pytest.raises(ValueError, match="2 -> 2"):
        realtime.HopSession(3, 128, sr=96000, locator=stub(3, model=calibration.FCNN(2, 3, hidden_layers=[4])))


def test_locator_must_live_on_the_session_device(no_gpu_calls):
    from onset_fingerprinting_amd import realtime
    with pytest.raises(ValueError, match="lives on"):
        realtime.HopSession(3, 128, sr=96000, locator=stub(3, device=1), device=0)


def test_without_a_locator_the_checks_do_not_run(no_gpu_calls):
    from onset_fingerprinting_amd import realtime
    with pytest.raises(AssertionError, match="GPU call"):  # straight to the library, as before
        realtime.HopSession(3, 128, sr=96000, backtrack=True)


def test_ongoing_list_keeps_aliases_as_one_object():
    from onset_fingerprinting_amd import _lib
    from onset_fingerprinting_amd import multilateration as ml
    st = _lib.LocateState()
    st.n_groups = 3
    for g, (n, alias, s, o) in enumerate([(2, 0, (1, 2), (10, 20)), (2, 1, (1, 2), (10, 20)), (1, 0, (0,), (30,))]):
        st.len[g], st.alias[g] = n, alias
        for k in range(n):
            st.sensors[g][k], st.onsets[g][k] = s[k], o[k]
    out = ml.ongoing_list(st)
    assert out == [([1, 2], [10, 20]), ([1, 2], [10, 20]), ([0], [30])]
    assert out[0] is out[1] and out[1] is not out[2]
    with pytest.raises(_lib.OnsetFPError, match="overflow"):
        ml.check_locate_flags(_lib.LOCF_GROUPS, "test")
    ml.check_locate_flags(0, "test")


def test_fixture_holds_what_its_generator_promises():
    g = load_golden("g25_hoplocate")  # allow_pickle=False
    cases = json.loads(str(g["cases"]))
    assert cases == ["rt3_fast3", "rt3_realtime", "air4_fast3", "air4_default"]
    for c in cases:
        args = json.loads(str(g[f"{c}/args"]))
        audio = g[f"{c}/audio"]
        assert audio.dtype == np.float32 and audio.shape[1] == len(args["layout"]["sensor_locations"])
        assert 96000 <= len(audio) <= 160000 and len(audio) % args["hop"] == 0
        H = len(g[f"{c}/hops"])
        assert g[f"{c}/onsets"].shape == (H, audio.shape[1])
        first = int(g[f"{c}/onsets"][0][g[f"{c}/onsets"][0] >= 0].min())
        assert first >= (100000 if c == "rt3_realtime" else 1500)
        for mode in ("audio", "plain"):
            res = g[f"{c}/{mode}/res"]
            assert res.shape == (H, 3) and res[:, 0].sum() >= 10
            assert np.isfinite(res[res[:, 0] == 1]).all()
            assert np.array_equal(g[f"{c}/{mode}/fed"] + g[f"{c}/{mode}/dropped"], g[f"{c}/n_onsets"])
            assert g[f"{c}/{mode}/n_groups"].max() <= 64 and g[f"{c}/{mode}/len"].max() <= 8
        if c.startswith("air4"):
            assert g[f"{c}/audio/swaps"] >= 1 and g[f"{c}/audio/dropped"].sum() >= 1
    assert g["air4_fast3/audio/len"].max() >= 4  # groups longer than three are carried along
    assert g["rt3_fast3/audio/n_groups"].max() >= 2
