#!/usr/bin/env python3
"""Golden vectors g25_hoplocate: the reference's realtime loop (realtime/audio.py:62-74, detect_hits) on synthetic
recordings -- its own AmplitudeOnsetDetector per hop, the hop's onsets sorted by sample, its own
Multilaterate3D.locate per onset until one returns a position -- with the ring as rec_audio and without.

Run in the build container only (after `make -C oracle ref`):   python tests/golden/make_golden_hoplocate.py

Contents, per case <c> in cases (a JSON list under "cases"):
  <c>/args       JSON: layout (Multilaterate3D arguments), hop, detector (AmplitudeOnsetDetector arguments), sr
  <c>/audio      [N, C] float32 (samples are multiples of 2^-12, which keeps the file small)
  <c>/hops       [H] int64: the hops that carried onsets
  <c>/n_onsets   [H] int64;  <c>/channels, <c>/onsets [H, C] int64 (-1 beyond n_onsets), in the detector's order
  and per mode <m> in (audio, plain):
  <c>/<m>/res      [H, 3] float64 = (located?, x, y) (NaN when nothing was located)
  <c>/<m>/fed      [H] int64 onsets given to locate;  <c>/<m>/dropped [H] int64 onsets after the one that located
  <c>/<m>/n_groups [H] int64, <c>/<m>/len [H, G] int64, <c>/<m>/sensors, <c>/<m>/onsets [H, G, M] int64 (-1 padded):
                   `ongoing` after the hop
  <c>/<m>/swaps    int64: calls of locate that swapped
"""
import contextlib
import io
import json
import sys
import warnings
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
REPO = HERE.parents[1]
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(REPO))

from _refload import load_reference  # noqa: E402
from make_golden_locate import LAYOUTS, _Ring, strikes, write_npz  # noqa: E402

warnings.filterwarnings("ignore")

RT = dict(hipass_freq=0, fast_ar=(0.3, 800), slow_ar=(8000, 8000), on_threshold=0.45, off_threshold=0.45,
          cooldown=1323, backtrack=False)  # realtime/audio.py:39-52
RT_FAST3 = dict(RT, fast_ar=(3.0, 800))
PERIOD, BURST = 3000, 600

CASES = [
    # name, layout, hop, detector arguments, samples, first strike
    ("rt3_fast3", "rt3", 128, RT_FAST3, 96000, 1500),
    ("rt3_realtime", "rt3", 128, RT, 160000, 101500),  # these arguments are reproducible from the first second on
    ("air4_fast3", "air4", 256, RT_FAST3, 96000, 1500),
    ("air4_default", "air4", 128, {}, 96000, 1500),
]


def recording(m, rng, n, first):
    C = len(m.sensor_locs)
    audio = np.zeros((n, C), np.float64)
    count = (n - first - 2 * PERIOD) // PERIOD
    pts = strikes(rng, count, m.radius)
    t = np.arange(BURST)
    for h, p in enumerate(pts):
        t0 = first + h * PERIOD
        for ch in range(C):
            s = m.sensor_locs[ch]
            d = np.sqrt((p[0] - s[0]) ** 2 + (p[1] - s[1]) ** 2 + s[2] ** 2)
            on = t0 + int(round(d / m.c * m.sr))
            f = (3000.0 + 700.0 * ch) * m.sr / 96000
            audio[on:on + BURST, ch] += 0.8 * np.exp(-t / 120.0) * np.sin(2 * np.pi * f / m.sr * t + 0.3 * h)
        if h % 4 == 3:  # a spurious onset between strikes
            ch = int(rng.integers(0, C))
            audio[t0 + 1700:t0 + 1700 + BURST, ch] += 0.5 * np.exp(-t / 120.0) * np.sin(2 * np.pi * 0.04 * t)
    return (np.round(audio * 4096) / 4096).astype(np.float32), count


def replay(ref, ml, layout, hop, det_kw, audio, with_audio):
    """detect_hits (realtime/audio.py:62-74) hop by hop; the ring is written before it (audio.py:97)."""
    C = audio.shape[1]
    od = ref.detection.AmplitudeOnsetDetector(C, hop, sr=layout["sr"], **det_kw)
    m = ml.Multilaterate3D(**layout)
    rows, current_index, swaps = [], 0, 0
    for h in range(len(audio) // hop):
        block = np.ascontiguousarray(audio[h * hop:(h + 1) * hop])
        ring = _Ring(audio, (h + 1) * hop)
        c, d, _ = od(block)
        if len(c) > 0:
            d = [current_index + x for x in d]
            idx = np.argsort(d)
            res, fed = None, 0
            for i in idx:
                fed += 1
                buf = io.StringIO()
                with contextlib.redirect_stdout(buf):
                    res = m.locate(c[i], d[i], ring if with_audio else None)
                swaps += buf.getvalue().count("swapping")
                if res is not None:
                    break
            rows.append(dict(hop=h, channels=[int(v) for v in c], onsets=[int(v) for v in d],
                             res=(0.0, np.nan, np.nan) if res is None else (1.0, float(res[0]), float(res[1])),
                             fed=fed, dropped=len(c) - fed,
                             ongoing=[([int(v) for v in g[0]], [int(v) for v in g[1]]) for g in m.ongoing]))
        current_index += hop
    return rows, swaps


def main():
    ref = load_reference()
    from onset_fingerprinting import multilateration as ml
    rng = np.random.default_rng(25)
    out = {"cases": np.array(json.dumps([c[0] for c in CASES]))}
    for name, lay, hop, det_kw, n, first in CASES:
        layout = LAYOUTS[lay]
        audio, n_strikes = recording(ml.Multilaterate3D(**layout), rng, n, first)
        C = audio.shape[1]
        out[f"{name}/args"] = np.array(json.dumps(dict(layout=layout, hop=hop, detector=det_kw, sr=layout["sr"])))
        out[f"{name}/audio"] = audio
        for mode, with_audio in (("audio", True), ("plain", False)):
            rows, swaps = replay(ref, ml, layout, hop, det_kw, audio, with_audio)
            H = len(rows)
            G = max(len(r["ongoing"]) for r in rows)
            M = max(len(g[0]) for r in rows for g in r["ongoing"])
            if mode == "audio":
                ch = np.full((H, C), -1, np.int64)
                on = np.full((H, C), -1, np.int64)
                for k, r in enumerate(rows):
                    ch[k, :len(r["channels"])] = r["channels"]
                    on[k, :len(r["onsets"])] = r["onsets"]
                out[f"{name}/hops"] = np.array([r["hop"] for r in rows], np.int64)
                out[f"{name}/n_onsets"] = np.array([len(r["channels"]) for r in rows], np.int64)
                out[f"{name}/channels"], out[f"{name}/onsets"] = ch, on
            else:  # the detector does not depend on the locator
                assert np.array_equal(out[f"{name}/hops"], [r["hop"] for r in rows])
            ln = np.full((H, G), -1, np.int64)
            gs = np.full((H, G, M), -1, np.int64)
            go = np.full((H, G, M), -1, np.int64)
            for k, r in enumerate(rows):
                for q, (s, o) in enumerate(r["ongoing"]):
                    ln[k, q] = len(s)
                    gs[k, q, :len(s)] = s
                    go[k, q, :len(o)] = o
            res = np.array([r["res"] for r in rows], np.float64)
            dropped = np.array([r["dropped"] for r in rows], np.int64)
            out[f"{name}/{mode}/res"] = res
            out[f"{name}/{mode}/fed"] = np.array([r["fed"] for r in rows], np.int64)
            out[f"{name}/{mode}/dropped"] = dropped
            out[f"{name}/{mode}/n_groups"] = np.array([len(r["ongoing"]) for r in rows], np.int64)
            out[f"{name}/{mode}/len"], out[f"{name}/{mode}/sensors"], out[f"{name}/{mode}/onsets"] = ln, gs, go
            out[f"{name}/{mode}/swaps"] = np.array(swaps, np.int64)
            located = int(res[:, 0].sum())
            print(f"{name}/{mode}: {n_strikes} strikes, {int(out[f'{name}/n_onsets'].sum())} onsets in {H} hops, "
                  f"located {located}, swaps {swaps}, dropped {int(dropped.sum())}, longest ongoing {G}, "
                  f"largest group {M}")
            # a later edit must not empty the fixture
            assert located >= 10, (name, mode, located)
            assert G <= 64 and M <= 8, (name, mode, G, M)
            if lay == "air4" and with_audio:
                assert swaps >= 1 and dropped.sum() >= 1, (name, swaps, int(dropped.sum()))
    path = HERE / "g25_hoplocate.npz"
    write_npz(path, out)
    size = path.stat().st_size
    print(f"wrote {path} ({size} bytes)")
    assert size < (HERE / "g6_stft.npz").stat().st_size, "the fixture must stay smaller than g6_stft.npz"


if __name__ == "__main__":
    main()
