"""GPU parity of Multilaterate3D.locate as device code (csrc/ofp_locate_dev.h): the replay entry
``Multilaterate3D.locate_stream_device`` against the committed reference trace (golden g22) and the host state
machine, and ``realtime.HopSession(locator=...)`` -- locate inside the hop's graph, both graph forms -- against the
reference's realtime loop run hop by hop (golden g25) and against the host-driven path."""
import json
import os

import numpy as np
import pytest
import torch

from tests.conftest import load_golden

pytestmark = pytest.mark.gpu

ROOT_TOL = 1e-6  # cm; one sample of lag moves a position by about 0.09 cm


def g22():
    return load_golden("g22_locate")


def g25():
    return load_golden("g25_hoplocate")


CASES = ["rt3_fast3", "rt3_realtime", "air4_fast3", "air4_default"]


class Ring:
    """rec_audio over a recording: .counter samples written, [-k:] the last k rows."""

    def __init__(self, audio, counter):
        self.audio, self.counter = audio, counter

    def __getitem__(self, idx):
        return self.audio[: self.counter][idx]


class SessionRing:
    """rec_audio over a session's device ring (rows before sample 0 are the zeros it was created with)."""

    def __init__(self, sess):
        self.sess, self.counter = sess, sess.current_index

    def __getitem__(self, idx):
        assert idx.stop is None and idx.step is None and idx.start < 0
        return self.sess.audio(-idx.start)


def rt3():
    from onset_fingerprinting_amd import multilateration as ml
    return ml.Multilaterate3D(**json.loads(str(g22()["m3d/rt3/args"])))


def plain(ongoing):
    return [(list(s), list(o)) for s, o in ongoing]


def golden_ongoing(g, case, mode, k):
    out = []
    for q in range(int(g[f"{case}/{mode}/n_groups"][k])):
        n = int(g[f"{case}/{mode}/len"][k, q])
        out.append(([int(v) for v in g[f"{case}/{mode}/sensors"][k, q, :n]],
                    [int(v) for v in g[f"{case}/{mode}/onsets"][k, q, :n]]))
    return out


def session(case, locator=True, with_audio=True, model=None, **kw):
    from onset_fingerprinting_amd import multilateration as ml
    from onset_fingerprinting_amd import realtime
    g = g25()
    args = json.loads(str(g[f"{case}/args"]))
    det = {k: (tuple(v) if isinstance(v, list) else v) for k, v in args["detector"].items()}
    m = ml.Multilaterate3D(**args["layout"], model=model)
    audio = g[f"{case}/audio"]
    kw.setdefault("ring_seconds", 1.0)
    sess = realtime.HopSession(audio.shape[1], args["hop"], sr=args["sr"], n_fft=2048,
                               locator=m if locator else None, locate_with_audio=with_audio, **det, **kw)
    return sess, m, audio, args["hop"]


def same_location(got, want_row, k):
    assert (got is not None) == bool(want_row[0]), k
    if got is not None:
        assert np.abs(np.array(got, np.float64) - want_row[1:]).max() < ROOT_TOL, k


# ---- 1: the replay entry against the committed reference trace ----------------------------------------------

@pytest.mark.parametrize("with_audio", [True, False])
def test_replay_matches_the_reference_trace_call_for_call(with_audio):
    g = g22()
    m = rt3()
    audio = g["trace/audio"]
    want = g["trace/res_audio" if with_audio else "trace/res_plain"]
    sens, ons, cnt = g["trace/sensor"], g["trace/onset"], g["trace/counter"]
    found, xy, ongoing = m.locate_stream_device(sens, ons, cnt, audio if with_audio else None)
    assert m.ongoing == []  # untouched
    assert np.array_equal(found, want[:, 0].astype(bool)), np.flatnonzero(found != want[:, 0].astype(bool))[:10]
    assert found.sum() >= 10
    assert np.abs(xy[found] - want[found, 1:]).max() < ROOT_TOL
    assert np.isnan(xy[~found]).all()
    for c, o, n in zip(sens, ons, cnt):  # the host state machine fed the same calls
        m.locate(int(c), int(o), Ring(audio, int(n)) if with_audio else None)
    assert plain(ongoing) == plain(m.ongoing)


# ---- 2: the session against the reference's realtime loop, both graph forms ---------------------------------

@pytest.mark.parametrize("with_audio", [True, False])
@pytest.mark.parametrize("form", ["fused", "nodes"])
@pytest.mark.parametrize("case", CASES)
def test_session_matches_the_reference_hop_by_hop(case, form, with_audio, monkeypatch):
    monkeypatch.setenv("OFP_HOP_GRAPH", form)
    g = g25()
    mode = "audio" if with_audio else "plain"
    sess, m, audio, B = session(case, with_audio=with_audio)
    hops = {int(h): k for k, h in enumerate(g[f"{case}/hops"])}
    seen = located = 0
    for h in range(len(audio) // B):
        r = sess(audio[h * B:(h + 1) * B])
        k = hops.get(h)
        if k is None:
            assert len(r["onsets"]) == 0 and r["location"] is None and r["fed"] == 0 and r["dropped"] == 0, h
            continue
        n = int(g[f"{case}/n_onsets"][k])
        # the precondition: the detector's onsets are the reference's
        assert np.array_equal(r["channels"], g[f"{case}/channels"][k, :n]), h
        assert np.array_equal(r["onsets"], g[f"{case}/onsets"][k, :n]), h
        same_location(r["location"], g[f"{case}/{mode}/res"][k], h)
        assert r["fed"] == g[f"{case}/{mode}/fed"][k] and r["dropped"] == g[f"{case}/{mode}/dropped"][k], h
        assert plain(sess.ongoing) == golden_ongoing(g, case, mode, k), h
        seen += 1
        located += r["location"] is not None
    assert seen == len(hops) and located == int(g[f"{case}/{mode}/res"][:, 0].sum()) >= 10
    assert m.ongoing == []
    sess.close()


# ---- 3: the session against the host-driven path --------------------------------------------------------------

def host_driven(sess, m, hop_result, with_audio):
    """detect_hits on the host: a locator-less session's onsets through Multilaterate3D.locate."""
    res, fed = None, 0
    order = np.argsort(hop_result["onsets"], kind="stable")
    for i in order:
        fed += 1
        res = m.locate(int(hop_result["channels"][i]), int(hop_result["onsets"][i]),
                       SessionRing(sess) if with_audio else None)
        if res is not None:
            break
    return res, fed, len(order) - fed


@pytest.mark.parametrize("with_audio", [True, False])
@pytest.mark.parametrize("case", CASES)
def test_session_matches_the_host_driven_path(case, with_audio):
    dev, m_dev, audio, B = session(case, with_audio=with_audio)
    host, m, _, _ = session(case, locator=False)
    located = 0
    for h in range(len(audio) // B):
        hop = audio[h * B:(h + 1) * B]
        r, q = dev(hop), host(hop)
        assert np.array_equal(r["onsets"], q["onsets"]) and np.array_equal(r["channels"], q["channels"])
        if len(q["onsets"]) == 0:
            assert r["location"] is None and r["fed"] == 0
            continue
        res, fed, dropped = host_driven(host, m, q, with_audio)
        assert (r["location"] is not None) == (res is not None), h
        if res is not None:
            assert np.abs(np.array(r["location"]) - np.array(res, np.float64)).max() < ROOT_TOL, h
            located += 1
        assert (r["fed"], r["dropped"]) == (fed, dropped), h
        assert plain(dev.ongoing) == plain(m.ongoing), h
    assert located >= 10
    dev.close()
    host.close()


# ---- 4: the model path ------------------------------------------------------------------------------------

def seeded_model():
    from onset_fingerprinting_amd import calibration
    torch.manual_seed(5)
    model = calibration.FCNN(2, 2, hidden_layers=[16, 16])
    model.eval()
    return model


@pytest.mark.parametrize("form", ["fused", "nodes"])
def test_model_path_uses_the_fcnn(form, monkeypatch):
    monkeypatch.setenv("OFP_HOP_GRAPH", form)
    model = seeded_model()
    dev, _, audio, B = session("rt3_fast3", model=model)
    host, m, _, _ = session("rt3_fast3", locator=False, model=model)
    located = 0
    for h in range(len(audio) // B):
        hop = audio[h * B:(h + 1) * B]
        r, q = dev(hop), host(hop)
        if len(q["onsets"]) == 0:
            continue
        res, fed, dropped = host_driven(host, m, q, True)
        assert (r["location"] is not None) == (res is not None), h
        if res is not None:
            got, want = np.array(r["location"]), np.array(res, np.float64)
            assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max(), h
            located += 1
        assert (r["fed"], r["dropped"]) == (fed, dropped), h
        assert plain(dev.ongoing) == plain(m.ongoing), h
    assert located >= 10
    # the replay entry takes the same network
    g = g22()
    mm = rt3()
    mm.model = model
    found, xy, _ = mm.locate_stream_device(g["trace/sensor"], g["trace/onset"], g["trace/counter"], g["trace/audio"])
    k = int(np.flatnonzero(found)[0])
    ref = rt3()
    ref.model = model
    for c, o, n in zip(g["trace/sensor"][:k + 1], g["trace/onset"][:k + 1], g["trace/counter"][:k + 1]):
        res = ref.locate(int(c), int(o), Ring(g["trace/audio"], int(n)))
    assert np.abs(xy[k] - np.array(res, np.float64)).max() <= 1e-5 * np.abs(np.array(res)).max()
    dev.close()
    host.close()


# ---- 5, 6, 7: ring wrap, reset, non-interference -----------------------------------------------------------

def run(sess, audio, B):
    rows = []
    for h in range(len(audio) // B):
        r = sess(audio[h * B:(h + 1) * B])
        rows.append((r["onsets"].tolist(), r["channels"].tolist(), r["location"], r["located_group"], r["fed"],
                     r["dropped"], plain(sess.ongoing) if len(r["onsets"]) else None))
    return rows


@pytest.mark.parametrize("case", ["rt3_fast3", "air4_fast3"])
def test_a_ring_just_above_the_minimum_gives_the_same_bits(case):
    from onset_fingerprinting_amd import multilateration as ml
    long_ring, m, audio, B = session(case)
    want = run(long_ring, audio, B)
    rows = max(ml.longest_section(m.max_max_lags, B) + B, 2048) + 7  # not a multiple of the hop
    assert rows % B != 0
    short, _, _, _ = session(case, ring_seconds=rows / long_ring.sr)
    assert short.ring_samples == rows
    assert run(short, audio, B) == want
    assert sum(r[2] is not None for r in want) >= 10
    long_ring.close()
    short.close()


def test_reset_gives_the_same_results_again():
    sess, _, audio, B = session("air4_fast3")
    first = run(sess, audio, B)
    assert sess.ongoing != [] or any(r[2] is not None for r in first)
    sess.reset()
    assert sess.ongoing == []
    assert run(sess, audio, B) == first
    sess.close()


@pytest.mark.parametrize("form", ["fused", "nodes"])
def test_a_locator_does_not_change_the_rest_of_the_hop(form, monkeypatch):
    from onset_fingerprinting_amd import calibration
    monkeypatch.setenv("OFP_HOP_GRAPH", form)
    torch.manual_seed(3)
    clf = calibration.FCNN(40, 5, hidden_layers=[24])
    clf.eval()
    a, _, audio, B = session("air4_fast3", classifier=clf, want_rel=True)
    b, _, _, _ = session("air4_fast3", locator=False, classifier=clf, want_rel=True)
    for h in range(len(audio) // B):
        hop = audio[h * B:(h + 1) * B]
        r, q = a(hop), b(hop)
        assert "location" in r and "location" not in q
        assert np.array_equal(r["onsets"], q["onsets"]) and np.array_equal(r["channels"], q["channels"]), h
        for key in ("rel", "mel", "logits"):
            assert np.array_equal(r[key].view(np.uint32), q[key].view(np.uint32)), (key, h)
    a.close()
    b.close()


# ---- 8: overflow is reported, never silent ------------------------------------------------------------------

def test_overflow_sets_the_flag_and_leaves_the_device_usable():
    from onset_fingerprinting_amd import _lib
    m = rt3()
    # 70 onsets of one sensor at one sample: every call keeps all earlier groups (lag 0, sensor already in the
    # group) and adds a seed, so the 65th call needs a 65th group
    K = 70
    sens, ons, cnt = np.zeros(K, np.int32), np.full(K, 5000, np.int64), np.full(K, 5128, np.int64)
    found, _, ongoing = m.locate_stream_device(sens[:64], ons[:64], cnt[:64])
    assert not found.any() and len(ongoing) == 64  # exactly full is not an overflow
    with pytest.raises(_lib.OnsetFPError, match="overflow"):
        m.locate_stream_device(sens, ons, cnt)
    g = g22()  # the device and the locator still work
    found, _, _ = m.locate_stream_device(g["trace/sensor"], g["trace/onset"], g["trace/counter"])
    assert np.array_equal(found, g["trace/res_plain"][:, 0].astype(bool))


def test_refused_calls_and_long_sections_are_reported():
    from onset_fingerprinting_amd import _lib
    from onset_fingerprinting_amd import multilateration as ml
    m = rt3()
    audio = g22()["trace/audio"]
    # a sensor the locator does not have, and a counter beyond the recording: the kernel refuses the call
    with pytest.raises(_lib.OnsetFPError, match="refused"):
        m.locate_stream_device([0, 3], [5000, 5100], [5128, 5228])
    with pytest.raises(_lib.OnsetFPError, match="refused"):
        m.locate_stream_device([0, 1], [5000, 5100], [5128, len(audio) + 1], audio)
    # the second onset is fed 6 000 samples after the first: its section is longer than the kernel holds
    assert 11000 - 5000 + ml.lookaround + 1 > ml.LOCATE_MAX_SECTION
    with pytest.raises(_lib.OnsetFPError, match="section"):
        m.locate_stream_device([0, 1], [5000, 5100], [5128, 11000], audio)
    found, _, ongoing = m.locate_stream_device([0, 1], [5000, 5100], [5128, 5228], audio)  # still usable
    assert not found.any() and len(ongoing) >= 1


@pytest.mark.parametrize("form", ["fused", "nodes"])
def test_a_refused_locator_leaves_the_session_as_it_was(form, monkeypatch):
    """ofp_hop_set_locator refuses a locator whose network does not fit the workgroup's LDS (an argument check).  The
    session is still the locator-less one it was, then accepts a valid locator and gives the reference's positions
    and state hop by hop -- read through the C ABI, as HopSession does for a session created with `locator=`."""
    import ctypes

    from onset_fingerprinting_amd import _lib, calibration
    from onset_fingerprinting_amd import multilateration as ml
    monkeypatch.setenv("OFP_HOP_GRAPH", form)
    case, mode = "rt3_fast3", "audio"
    g = g25()
    sess, m, audio, B = session(case, locator=False)
    torch.manual_seed(5)
    wide = calibration.FCNN(2, 2, hidden_layers=[1024, 1024])  # two tiles of 16 x 1025 floats: 128 KiB and a bit
    wide.eval()
    m_wide = ml.Multilaterate3D(**json.loads(str(g[f"{case}/args"]))["layout"], model=wide)
    section = ml.longest_section(m.max_max_lags, B)
    mlp = m_wide._device_model("test")
    L = _lib.lib()
    with torch.cuda.device(sess.device):
        rc = L.ofp_hop_set_locator(sess.handle, ctypes.byref(m_wide.locator_struct(True, section, mlp)))
    assert rc != 0 and "bytes of LDS needed" in L.ofp_last_error().decode()
    assert "location" not in sess(audio[:B])  # still a session without a locator ...
    sess.reset()
    with torch.cuda.device(sess.device):  # ... that takes one
        _lib.check(L.ofp_hop_set_locator(sess.handle, ctypes.byref(m.locator_struct(True, section))),
                   "ofp_hop_set_locator")
    hops = {int(h): k for k, h in enumerate(g[f"{case}/hops"])}
    status, fed, dropped = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    xy, state, located = (ctypes.c_double * 2)(), _lib.LocateState(), 0
    for h in range(len(audio) // B):
        r = sess(audio[h * B:(h + 1) * B])
        k = hops.get(h)
        if k is None:
            assert len(r["onsets"]) == 0, h
            continue
        n = int(g[f"{case}/n_onsets"][k])
        assert np.array_equal(r["channels"], g[f"{case}/channels"][k, :n]), h
        assert np.array_equal(r["onsets"], g[f"{case}/onsets"][k, :n]), h
        _lib.check(L.ofp_hop_collect_location(sess.handle, ctypes.byref(status), xy, None, None, None,
                                              ctypes.byref(fed), ctypes.byref(dropped), None), "collect_location")
        same_location((xy[0], xy[1]) if status.value == 1 else None, g[f"{case}/{mode}/res"][k], h)
        assert fed.value == g[f"{case}/{mode}/fed"][k] and dropped.value == g[f"{case}/{mode}/dropped"][k], h
        _lib.check(L.ofp_hop_locator_state(sess.handle, ctypes.byref(state)), "locator_state")
        assert plain(ml.ongoing_list(state)) == golden_ongoing(g, case, mode, k), h
        located += status.value == 1
    assert located == int(g[f"{case}/{mode}/res"][:, 0].sum()) >= 10
    sess.close()
