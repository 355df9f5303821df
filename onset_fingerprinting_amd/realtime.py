"""Per-hop streaming on MI355X (BASELINE config 5): the data path of the reference's
realtime callback with everything between "a hop of samples arrives" and "onsets +
classifier outputs are on the host" in ONE captured hipGraph on device-resident state.

Reference call pattern:
  realtime/audio.py:96-97     copy the hop, write it into the 60 s ring buffer
  realtime/audio.py:62-74     ``self.od(audio)`` -> AmplitudeOnsetDetector.__call__ on the hop,
                              onset = current_index + delta
  multilateration.py:555-557  ``FCNN.call_np`` -> calibration.py:552-560
  realtime/recording.py:273-280  one rFFT frame of ``audio[-n_fft:]`` per hop

The sound-card I/O, VST effects, geometry solver and shared-memory plumbing of
``realtime/`` are out of scope; this module is the hot path
they call.  No CPU path: without libonsetfp.so or a gfx950 GPU every call raises.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import HopConfig, check
from .data import mel_filterbank
from .detection import ONSET_DTYPE, _DeviceDetector

# the detector arguments of the reference's realtime setup (realtime/audio.py:39-52)
REALTIME_DETECTOR_KWARGS = dict(hipass_freq=0, fast_ar=(0.3, 800), slow_ar=(8000, 8000), on_threshold=0.45,
                                off_threshold=0.45, cooldown=1323, backtrack=False)


def _band_csr(dense):
    lo, ln, off, w = [], [], [], []
    for b in range(dense.shape[0]):
        nz = np.nonzero(dense[b])[0]
        if len(nz) == 0:
            lo.append(0), ln.append(0), off.append(len(w))
            continue
        lo.append(int(nz[0])), ln.append(int(nz[-1] - nz[0] + 1)), off.append(len(w))
        w.extend(dense[b, nz[0]:nz[-1] + 1].tolist())
    return (np.asarray(lo, np.int32), np.asarray(ln, np.int32), np.asarray(off, np.int32),
            np.asarray(w if w else [0.0], np.float32))


def regress_hold_hops(block_size, frame_length, pre_samples, max_distance):
    """K: a kept group is evaluated at most K hops after the hop that closes it ("The window
    regressor in the hop").  The group anchored at sample a closes at a hop c with c * B > a + B, and its window
    (start <= a + max_distance - pre_samples) is complete at the hop d with d * B < start + frame_length + B, so
    d - c < (max_distance + frame_length - pre_samples) / B; one group closes per hop at most (max_distance >= B) and
    one is evaluated per hop, so a backlog never adds to that."""
    return max(0, -(-(max_distance + frame_length - pre_samples) // block_size) - 1)


def regress_pending_bound(block_size, frame_length, pre_samples, max_distance):
    """Most groups in the stage's FIFO at once: the groups closed in the K + 1 hops up to h.  At most one closes per
    hop, and their anchors lie in [(h - K - 1) * B - max_distance, (h - 1) * B), more than max_distance apart."""
    K = regress_hold_hops(block_size, frame_length, pre_samples, max_distance)
    return min(K + 1, (K * block_size + max_distance - 1) // (max_distance + 1) + 1)


def regress_ring_rows(block_size, frame_length, pre_samples, max_distance):
    """Rows the ring must hold: from the earliest start (anchor - pre_samples) to the end of the latest hop that can
    evaluate the group (anchor + max_distance + (K + 1) * B), the hop being written included."""
    K = regress_hold_hops(block_size, frame_length, pre_samples, max_distance)
    return max_distance + pre_samples + (K + 1) * block_size


def _check_regressor(what, model, n_signals, block_size, frame_length, pre_samples, max_distance, min_channels):
    """The argument errors of a regress stage that need no GPU -> (the model's arch, frame_length)."""
    from . import model as mdl
    arch = mdl.hop_regressor_arch(model, what)
    if arch.channels != n_signals:
        raise ValueError(f"{what}: the regressor takes {arch.channels} channels, the stream has {n_signals} signals")
    if frame_length is None:
        frame_length = arch.input_size
    if int(frame_length) != arch.input_size:
        raise ValueError(f"{what}: frame_length {frame_length}, the regressor's input_size is {arch.input_size}")
    if pre_samples < 0:
        raise ValueError(f"{what}: pre_samples {pre_samples} is negative")
    if max_distance < 0:
        raise ValueError(f"{what}: max_distance {max_distance} is negative")
    if not 1 <= min_channels <= n_signals:
        raise ValueError(f"{what}: min_channels {min_channels} outside 1..{n_signals}")
    return arch, int(frame_length)


def check_regress_flags(flags, what):
    """The regress stage's sticky flags are never silent."""
    if flags & _lib.REGF_QUEUE:
        raise _lib.OnsetFPError(f"{what}: the regress queue overflowed (more than {_lib.REG_QUEUE} groups pending; "
                                f"flags {flags})")
    if flags & _lib.REGF_BAD_ONSET:
        raise _lib.OnsetFPError(f"{what}: an onset was refused (channel out of range or negative sample; flags {flags})")


def regress_stream_device(model, audio, channels, onsets, block_size, frame_length=None, pre_samples=0,
                          max_distance=1000, min_channels=3, device=0):
    """What a ``HopSession(regressor=model)`` would have answered on a finished recording, in ONE launch
    (``ofp_regress_stream``): the stage's grouping state machine and model over ``audio`` [N, C] float32 (numpy or a
    CUDA tensor) and the onset list (``channels`` / ``onsets`` [K], absolute samples; fed sorted by sample, stable),
    hop by hop (N // block_size hops).  Returns a dict of per-hop arrays: ``hit`` bool [H], ``start`` int64 [H],
    ``group`` int64 [H, C], ``position`` float32 [H, n_out] (zeros where ``hit`` is False) and ``pending`` int32 [H],
    the FIFO's length before the hop's evaluation.  The ring and queue conditions of a session do not apply (the
    recording is resident); a queue overflow raises OnsetFPError."""
    what = "regress_stream_device"
    ad = audio if torch.is_tensor(audio) else torch.from_numpy(np.ascontiguousarray(audio, dtype=np.float32))
    if ad.dim() != 2:
        raise ValueError(f"{what}: audio must be [N, C], got {tuple(ad.shape)}")
    C = int(ad.shape[1])
    arch, frame_length = _check_regressor(what, model, C, block_size, frame_length, pre_samples, max_distance,
                                          min_channels)
    onsets = np.asarray(onsets, dtype=np.int64).reshape(-1)
    channels = np.asarray(channels, dtype=np.int32).reshape(-1)
    if len(onsets) != len(channels):
        raise ValueError(f"{what}: {len(channels)} channels for {len(onsets)} onsets")
    order = np.argsort(onsets, kind="stable")
    onsets, channels = onsets[order], channels[order]
    from . import model as mdl
    dev = torch.device("cuda", device) if not isinstance(device, torch.device) else device
    _lib.require_gpu(dev.index or 0)
    L = _lib.lib()
    ad = ad.to(dev, torch.float32).contiguous()
    H = int(ad.shape[0]) // block_size
    with torch.cuda.device(dev):
        r, keep = mdl.hop_regressor_struct(model, dev, frame_length, pre_samples, max_distance, min_channels, what)
        ws_floats = int(L.ofp_regress_workspace_floats(ctypes.byref(r)))
        if ws_floats < 0:
            raise ValueError(_lib.last_error())
        ws = torch.empty(2 * ws_floats, dtype=torch.float32, device=dev) if ws_floats else None
        ch_d, on_d = torch.from_numpy(channels).to(dev), torch.from_numpy(onsets).to(dev)
        status = torch.zeros(H, dtype=torch.int32, device=dev)
        start = torch.zeros(H, dtype=torch.int64, device=dev)
        rows = torch.zeros((H, C), dtype=torch.int64, device=dev)
        y = torch.zeros((H, arch.n_out), dtype=torch.float32, device=dev)
        pending = torch.zeros(H, dtype=torch.int32, device=dev)
        flags = torch.zeros(1, dtype=torch.int32, device=dev)
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        check(L.ofp_regress_stream(ctypes.byref(r), ad.data_ptr(), ad.shape[0], block_size, ch_d.data_ptr(),
                                   on_d.data_ptr(), len(onsets), status.data_ptr(), start.data_ptr(), rows.data_ptr(),
                                   y.data_ptr(), pending.data_ptr(), flags.data_ptr(),
                                   ws.data_ptr() if ws is not None else None, stream), "ofp_regress_stream")
        del keep
    check_regress_flags(int(flags.item()), what)
    return dict(hit=status.cpu().numpy().astype(bool), start=start.cpu().numpy(), group=rows.cpu().numpy(),
                position=y.cpu().numpy(), pending=pending.cpu().numpy())


class HopSession:
    """One stream: ring buffer + detector + per-hop spectral fingerprint + classifier.

    ``session(hop)`` takes ``[block_size, n_signals]`` float32 and returns a dict with
    ``channels`` / ``onsets`` (absolute sample indices, as ``detect_hits`` forms them,
    audio.py:65), ``logits`` ``[n_signals, n_out]`` (None without a classifier), ``mel``
    ``[n_signals, n_mels]`` and, with ``want_rel``, the hop's relative envelope.

    ``locator``: a ``multilateration.Multilaterate3D`` on the session's device.  The hop's graph then also runs
    ``detect_hits`` (realtime/audio.py:62-74): the hop's onsets, sorted by sample, go through
    ``Multilaterate3D.locate`` on a device-resident copy of its state until one returns a position
    (``locate_with_audio``: with the ring as ``rec_audio``).  The result dict gains ``location`` (None or (x, y) in
    cm, as ``locate`` returns it), ``located_group`` (None or ([sensors], [onsets]) as ``trilaterate`` left it),
    ``fed`` (onsets given to the state machine) and ``dropped`` (onsets of the hop after the one that located: the
    reference returns at the first hit and never feeds them).  ``ongoing`` reads the state back.  The locator's own
    ``ongoing`` is not touched.

    ``locator`` may also be the planar ``multilateration.Multilaterate`` (``ofp_hop_set_locator_2d``): the stage then
    runs ``Multilaterate.locate``.  That class has no cross-correlation step, so ``locate_with_audio`` is ignored and
    no ring length is required.  ``location`` is the polar tuple (radius / drum radius, angle) ``locate`` returns,
    formed on the host from the device's Cartesian root; ``located_group``, ``fed``, ``dropped`` and ``ongoing`` are as
    above.

    ``regressor``: a ``model.CNN``, ``CCCNN`` or ``LCCCNN`` (eval semantics) on ``frame_length`` (default and only
    value: its ``input_size``) samples of every channel.  The hop's graph then also groups the stream's onsets as
    ``detection.find_onset_groups(max_distance, min_channels)`` would on the whole list, and runs the model on the
    window of the group whose last row the hop delivers (``data.FrameExtractor``, ``use_min_onset``, ``pre_samples``,
    no shift; at most one group per hop, after the locator stage).  The result dict gains ``hit``: None, or a dict
    with ``position`` float32 [n_out], ``group`` int64 [n_signals] (the group's row, -1 where a channel is missing)
    and ``start`` (the window's first sample).  INTEGRATION.md, "The window regressor in the hop", has the details.

    ``locator`` may finally be a ``multilateration.MultilateratePaired`` (``ofp_hop_set_locator_paired``), with
    ``tol``, ``left``, ``right`` (``locate_cc``'s) and ``max_distance``, ``min_channels`` (the grouping's): the hop's
    graph then groups the stream's onsets as for a regressor and runs ``locate_cc`` on the group whose window
    ``x[onset - left : onset + right]`` the hop completes.  The result dict gains ``location`` (None or the polar tuple
    ``locate_cc`` returns) and ``cc_hit``: None, or a dict with ``status`` (PAIRED_OK, or PAIRED_NEG_WINDOW for a
    window that starts below sample 0: no location), ``onset``, ``first``, ``group`` int64 [n_signals], ``lags`` int32
    [2] and ``cell``.  The locator's ``res`` is not touched; a regressor cannot be attached beside it.  The session
    keeps a reference to the locator, whose device tables it reads.  INTEGRATION.md, "The voting locator in the hop".
    """

    def __init__(self, n_signals, block_size=128, sr=96000, n_fft=2048, n_mels=40, classifier=None,
                 ring_seconds=60.0, want_rel=False, device=0, floor=-70.0, hipass_freq=2000.0,
                 fast_ar=(3.0, 383.0), slow_ar=(2205.0, 2205.0), on_threshold=0.5, off_threshold=0.1,
                 cooldown=1323, backtrack=False, backtrack_buffer_size=None, backtrack_smooth_size=5,
                 onset_strength=None, locator=None, locate_with_audio=True, regressor=None, frame_length=None,
                 pre_samples=0, max_distance=1000, min_channels=3, tol=2, left=0, right=256):
        ring_rows = max(int(round(ring_seconds * sr)), n_fft, block_size)  # realtime/config.py:45,59
        self._paired = False
        if locator is not None:
            from . import multilateration as ml
            self._paired = isinstance(locator, ml.MultilateratePaired)
        if self._paired:  # argument errors before any GPU call, from the locator's host attributes
            what = "HopSession"
            if regressor is not None:
                raise ValueError("HopSession: locator=MultilateratePaired and regressor= are both grouping stages; one "
                                 "session runs one of them")
            if backtrack:
                raise ValueError("HopSession: a locator needs backtrack=False (a backtracked onset may lie behind the "
                                 "current hop)")
            locator.check_stage(what, n_signals, tol, left, right, max_distance, min_channels)
            want = device.index or 0 if isinstance(device, torch.device) else int(device)
            if (locator.device.index or 0) != want:
                raise ValueError(f"HopSession: the locator lives on {locator.device}, the session on device {want}")
            if max_distance < block_size:
                raise ValueError(f"HopSession: max_distance {max_distance} is shorter than one hop ({block_size} "
                                 "samples): two groups could close in one hop")
            bounds = (block_size, int(left) + int(right), int(left), max_distance)  # the regress stage's, F and pre
            if regress_pending_bound(*bounds) > _lib.REG_QUEUE:
                raise ValueError(f"HopSession: up to {regress_pending_bound(*bounds)} groups can be pending with these "
                                 f"parameters, the device queue holds {_lib.REG_QUEUE}")
            if ring_rows < regress_ring_rows(*bounds):
                raise ValueError(f"HopSession: the ring of {ring_rows} rows is too short for the oldest row a pending "
                                 f"window can still need plus one hop ({regress_ring_rows(*bounds)} rows)")
        if regressor is not None:  # argument errors before any GPU call
            what = "HopSession"
            if backtrack:
                raise ValueError("HopSession: a regressor needs backtrack=False (a backtracked onset may lie behind the "
                                 "current hop)")
            _, frame_length = _check_regressor(what, regressor, n_signals, block_size, frame_length, pre_samples,
                                               max_distance, min_channels)
            if max_distance < block_size:  # (the bounds below rest on it; the replay has no such condition)
                raise ValueError(f"HopSession: max_distance {max_distance} is shorter than one hop ({block_size} "
                                 "samples): two groups could close in one hop")
            bounds = (block_size, frame_length, pre_samples, max_distance)
            if regress_pending_bound(*bounds) > _lib.REG_QUEUE:
                raise ValueError(f"HopSession: up to {regress_pending_bound(*bounds)} groups can be pending with these "
                                 f"parameters, the device queue holds {_lib.REG_QUEUE}")
            if ring_rows < regress_ring_rows(*bounds):
                raise ValueError(f"HopSession: the ring of {ring_rows} rows is too short for the oldest row a pending "
                                 f"window can still need plus one hop ({regress_ring_rows(*bounds)} rows)")
        if locator is not None and not self._paired:  # argument errors before any GPU call
            if len(locator.sensor_locs) != n_signals:
                raise ValueError(f"HopSession: the locator has {len(locator.sensor_locs)} sensors, the session "
                                 f"{n_signals} signals")
            if backtrack:
                raise ValueError("HopSession: a locator needs backtrack=False (a backtracked onset may lie behind the "
                                 "current hop)")
            self._planar = isinstance(locator, ml.Multilaterate)
            if not self._planar:
                self._max_section = ml.longest_section(locator.max_max_lags, block_size)
                if locate_with_audio and (ring_rows < self._max_section + block_size
                                          or self._max_section > ml.LOCATE_MAX_SECTION):
                    raise ValueError(f"HopSession: the ring of {ring_rows} rows is too short for the longest section "
                                     f"({self._max_section} rows, at most {ml.LOCATE_MAX_SECTION}) plus one hop")
                ml.check_locator_model(locator.model, "HopSession")
            want = device.index or 0 if isinstance(device, torch.device) else int(device)
            if (locator.device.index or 0) != want:
                raise ValueError(f"HopSession: the locator lives on {locator.device}, the session on device {want}")
        L = _lib.lib()
        self.n_signals, self.block_size, self.sr, self.n_fft, self.n_mels = n_signals, block_size, sr, n_fft, n_mels
        if backtrack_buffer_size is None:
            backtrack_buffer_size = 2 * block_size  # audio.py:50
        self.d = _DeviceDetector(n_signals, block_size, floor, hipass_freq, fast_ar, slow_ar, on_threshold,
                                 off_threshold, cooldown, backtrack, backtrack_buffer_size, backtrack_smooth_size,
                                 sr, device)
        self.device = self.d.device
        lo, ln, off, w = _band_csr(mel_filterbank(sr, n_fft, n_mels))
        self._keep = (lo, ln, off, w)
        self.classifier = classifier
        mlp = classifier.device_mlp(self.device) if classifier is not None else None
        self.n_out = mlp.n_out if mlp is not None else 0
        cfg = HopConfig()
        cfg.n_fft = n_fft
        cfg.ring_samples = ring_rows
        cfg.n_mels = n_mels
        cfg.fb_lo, cfg.fb_len, cfg.fb_off, cfg.fb_w = (a.ctypes.data for a in (lo, ln, off, w))
        cfg.fb_nnz = len(w)
        cfg.mlp = mlp.handle if mlp is not None else None
        cfg.want_rel = int(bool(want_rel))
        self.want_rel = bool(want_rel)
        # per-hop onset strength of the channel mean (realtime/recording.py:273-311; PARITY UNPINNED: its two
        # trackers are loopmate.EMA_MinMaxTracker objects, loopmate is absent; see include/onsetfp.h).
        # onset_strength: None, or a dict with max_length / avg_length (the reference's undefined
        # config.MAX_LENGTH / AVG_LENGTH) and optionally ring, tg_win_length, ls_* / oe_* tracker constants
        self.onset_strength = None
        if onset_strength is not None:
            o = dict(ring=int(np.ceil(max(int(round(ring_seconds * sr)), n_fft) / block_size)), ls_max0=10.0,
                     ls_minmax=0.0, ls_alpha=0.0005, oe_min0=0.0, oe_minmin=0.0, oe_max0=1.0, oe_alpha=0.001)
            o.update(onset_strength)
            cfg.strength = 1
            cfg.strength_ring, cfg.max_length, cfg.avg_length = int(o["ring"]), int(o["max_length"]), int(o["avg_length"])
            cfg.ls_max0, cfg.ls_minmax, cfg.ls_alpha = o["ls_max0"], o["ls_minmax"], o["ls_alpha"]
            cfg.oe_min0, cfg.oe_minmin, cfg.oe_max0, cfg.oe_alpha = o["oe_min0"], o["oe_minmin"], o["oe_max0"], o["oe_alpha"]
            # tg_win_length (config.TG_WIN_LENGTH = 1024 upstream): the tempogram frame per hop as well
            # (recording.py:313-327); needs tg_win_length <= ring
            cfg.tg_win_length = int(o.get("tg_win_length") or 0)
            self.onset_strength = o
        self.ring_samples = int(cfg.ring_samples)
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            check(L.ofp_hop_create(self.d.handle, ctypes.byref(cfg), ctypes.byref(h)), "ofp_hop_create")
        self.handle = h
        self._L = L
        self._n = ctypes.c_int64()
        self._rec = np.zeros(max(n_signals, 1), dtype=ONSET_DTYPE)
        self._logits = np.zeros((n_signals, max(self.n_out, 1)), dtype=np.float32)
        self._mel = np.zeros((n_signals, n_mels), dtype=np.float32)
        self._rel = np.zeros((block_size, n_signals), dtype=np.float32)
        self._sg = np.zeros(4 + (int(cfg.tg_win_length) if onset_strength is not None else 0), dtype=np.float32)
        self.current_index = 0  # audio.py:120
        self._group = None  # the HopSessionGroup that carries this session's hops, if any
        self.locator = locator
        if self._paired:
            try:
                p = locator.paired_struct(tol, left, right, max_distance, min_channels)  # (points into the locator's
                with torch.cuda.device(self.device):                                     #  tables: self.locator)
                    check(L.ofp_hop_set_locator_paired(self.handle, ctypes.byref(p)), "ofp_hop_set_locator_paired")
            except Exception:
                self.close()
                raise
            self.tol, self.left, self.right = tol, left, right
            self.max_distance, self.min_channels = max_distance, min_channels
            self._cc_i = [ctypes.c_int32() for _ in range(5)]  # hit, status, first, cell, flags
            self._cc_onset = ctypes.c_int64()
            self._cc_row = np.zeros(n_signals, dtype=np.int64)
            self._cc_lags = np.zeros(2, dtype=np.int32)
            self._cc_xy = np.zeros(2, dtype=np.float64)
            self._cc_rphi = np.zeros(2, dtype=np.float64)
        elif locator is not None:
            try:
                if self._planar:
                    entry, loc = "ofp_hop_set_locator_2d", locator.locator_struct()
                else:
                    self._loc_mlp = locator._device_model("HopSession")  # kept alive with the session
                    entry, loc = "ofp_hop_set_locator", locator.locator_struct(locate_with_audio, self._max_section,
                                                                               self._loc_mlp)
                with torch.cuda.device(self.device):
                    check(getattr(L, entry)(self.handle, ctypes.byref(loc)), entry)
            except Exception:
                self.close()
                raise
            self._loc_i = [ctypes.c_int32() for _ in range(5)]  # status, n_members, fed, dropped, flags
            self._loc_xy = (ctypes.c_double * 2)()
            self._loc_sens = (ctypes.c_int32 * _lib.LOCS_MEMBERS)()
            self._loc_on = (ctypes.c_int64 * _lib.LOCS_MEMBERS)()
        self.regressor = regressor
        if regressor is not None:  # (after the locator: its stage runs first)
            from . import model as mdl
            try:
                with torch.cuda.device(self.device):
                    r, keep = mdl.hop_regressor_struct(regressor, self.device, frame_length, pre_samples, max_distance,
                                                       min_channels, "HopSession")
                    check(L.ofp_hop_set_regressor(self.handle, ctypes.byref(r)), "ofp_hop_set_regressor")
                    del keep  # (the session has copied the parameters)
            except Exception:
                self.close()
                raise
            self.frame_length, self.pre_samples = frame_length, pre_samples
            self.max_distance, self.min_channels = max_distance, min_channels
            self._hit_i = [ctypes.c_int32(), ctypes.c_int64(), ctypes.c_int32()]  # status, start, flags
            self._hit_row = np.zeros(n_signals, dtype=np.int64)
            self._hit_y = np.zeros(r.n_out, dtype=np.float32)

    def _hit(self, out):
        status, start, flags = self._hit_i
        check(self._L.ofp_hop_collect_hit(self.handle, ctypes.byref(status), ctypes.byref(start),
                                          self._hit_row.ctypes.data, self._hit_y.ctypes.data, ctypes.byref(flags)),
              "ofp_hop_collect_hit")
        check_regress_flags(flags.value, "HopSession")
        out["hit"] = (dict(position=self._hit_y.copy(), group=self._hit_row.copy(), start=int(start.value))
                      if status.value == 1 else None)
        return out

    def _cc_hit(self, out):
        from . import multilateration as ml
        hit, status, first, cell, flags = self._cc_i
        check(self._L.ofp_hop_collect_cc_hit(self.handle, ctypes.byref(hit), ctypes.byref(status),
                                             ctypes.byref(self._cc_onset), ctypes.byref(first), self._cc_row.ctypes.data,
                                             self._cc_lags.ctypes.data, ctypes.byref(cell), self._cc_xy.ctypes.data,
                                             self._cc_rphi.ctypes.data, ctypes.byref(flags)), "ofp_hop_collect_cc_hit")
        check_regress_flags(flags.value, "HopSession")
        out["location"] = out["cc_hit"] = None
        if hit.value == 1:
            out["cc_hit"] = dict(status=int(status.value), onset=int(self._cc_onset.value), first=int(first.value),
                                 group=self._cc_row.copy(), lags=self._cc_lags.copy(), cell=int(cell.value))
            if status.value == ml.PAIRED_OK:  # cartesian_to_polar of the cell, as locate_cc returns it
                out["location"] = (np.float64(self._cc_rphi[0]), np.float64(self._cc_rphi[1]))
        return out

    def _location(self, out):
        from . import multilateration as ml
        status, n, fed, dropped, flags = self._loc_i
        check(self._L.ofp_hop_collect_location(self.handle, ctypes.byref(status), self._loc_xy, ctypes.byref(n),
                                               self._loc_sens, self._loc_on, ctypes.byref(fed), ctypes.byref(dropped),
                                               ctypes.byref(flags)), "ofp_hop_collect_location")
        ml.check_locate_flags(flags.value, "HopSession")
        hit = status.value == 1
        out["location"] = (np.float64(self._loc_xy[0]), np.float64(self._loc_xy[1])) if hit else None
        if hit and self._planar:  # Multilaterate.trilaterate's last step
            out["location"] = ml.cartesian_to_polar(*out["location"], self.locator.radius)
        out["located_group"] = (list(self._loc_sens[:n.value]), list(self._loc_on[:n.value])) if hit else None
        out["fed"], out["dropped"] = fed.value, dropped.value
        return out

    @property
    def ongoing(self):
        """The device state as the reference's ``ongoing`` of the locator's class: a list of ([sensors], [onsets])."""
        from . import multilateration as ml
        if self.locator is None:
            raise ValueError("HopSession.ongoing: the session has no locator")
        if self._paired:
            raise ValueError("HopSession.ongoing: the voting locator keeps groups, not the trilaterating state")
        st = _lib.LocateState()
        check(self._L.ofp_hop_locator_state(self.handle, ctypes.byref(st)), "ofp_hop_locator_state")
        return ml.ongoing_list(st)

    def close(self):
        if getattr(self, "_group", None) is not None:  # a member goes only after its group: the group's graph
            self._group.close()                        # holds the session's device pointers
        if getattr(self, "handle", None):
            self._L.ofp_hop_destroy(self.handle)
            self.handle = None
        self.d.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        check(self._L.ofp_hop_reset(self.handle), "ofp_hop_reset")
        self.current_index = 0

    def init_minmax_tracker(self, x):
        """AmplitudeOnsetDetector.init_minmax_tracker (detection.py:827-840)."""
        x = self._f32(x, None)
        if len(x):
            check(self._L.ofp_hop_warmup(self.handle, x.ctypes.data, len(x)), "ofp_hop_warmup")

    def _f32(self, x, rows):
        x = np.ascontiguousarray(x)
        if x.dtype != np.float32:
            # the reference's ctypes ndpointer rejects non-float32 input (detection.py:521-526)
            raise ctypes.ArgumentError(f"array must have data type float32, got {x.dtype}")
        if x.ndim != 2 or x.shape[1] != self.n_signals or (rows is not None and x.shape[0] != rows):
            raise ValueError(f"expected shape ({rows if rows is not None else 'n'}, {self.n_signals}), got {x.shape}")
        return x

    def submit(self, hop):
        hop = self._f32(hop, self.block_size)
        check(self._L.ofp_hop_submit(self.handle, hop.ctypes.data), "ofp_hop_submit")

    def collect(self):
        check(self._L.ofp_hop_collect(self.handle, ctypes.byref(self._n), self._rec.ctypes.data,
                                      self._logits.ctypes.data if self.n_out else None, self._mel.ctypes.data,
                                      self._rel.ctypes.data if self.want_rel else None,
                                      self._sg.ctypes.data if self.onset_strength else None), "ofp_hop_collect")
        k = min(int(self._n.value), self.n_signals)
        self.current_index += self.block_size
        out = dict(channels=self._rec["channel"][:k].astype(np.int64), onsets=self._rec["sample"][:k].copy(),
                    logits=self._logits.copy() if self.n_out else None, mel=self._mel.copy(),
                    rel=self._rel.copy() if self.want_rel else None,
                    # {flux, normalised, moving max, moving mean} of recording.py:296-311
                    strength=self._sg[:4].copy() if self.onset_strength else None,
                    # recording.py:313-327 (None unless onset_strength has tg_win_length)
                    tempogram=self._sg[4:].copy() if self.onset_strength and len(self._sg) > 4 else None)
        if self.regressor is not None:
            self._hit(out)
        if self.locator is None:
            return out
        if self._paired:
            return self._cc_hit(out)
        if k == 0:  # the stage did not run: nothing to read
            out.update(location=None, located_group=None, fed=0, dropped=0)
            return out
        return self._location(out)

    def __call__(self, hop):
        self.submit(hop)
        return self.collect()

    def push_raw(self, hop):
        """`__call__` without building the result dict (latency measurements): returns the number
        of onsets; the outputs stay in the session's host arrays."""
        check(self._L.ofp_hop_push(self.handle, hop.ctypes.data, ctypes.byref(self._n), self._rec.ctypes.data,
                                   self._logits.ctypes.data if self.n_out else None, self._mel.ctypes.data,
                                   self._rel.ctypes.data if self.want_rel else None,
                                   self._sg.ctypes.data if self.onset_strength else None), "ofp_hop_push")
        self.current_index += self.block_size
        return int(self._n.value)

    def audio(self, n):
        """``rec_audio[-n:]`` (the last n rows of the device ring buffer, oldest first)."""
        out = np.empty((int(n), self.n_signals), dtype=np.float32)
        check(self._L.ofp_hop_ring_read(self.handle, int(n), out.ctypes.data), "ofp_hop_ring_read")
        return out


class HopSessionGroup:
    """S streams per hop period in ONE graph launch (``ofp_hop_group_*``): several drums, players or clients whose
    hops arrive on the same clock.

    ``sessions``: ``HopSession`` objects on one device with the same ``n_fft`` and channel count that agree on
    having a locator, on having a voting locator (``MultilateratePaired``; locators, ``tol``, ``left`` and ``right`` may
    differ), on having a regressor (its architecture may differ) and on having the onset strength; everything else (block size, ``sr``, detector arguments, ring
    length, ``want_rel``, ``n_mels``, classifier, the locator's geometry and model) may differ.  They may be warmed
    up or mid-stream.  Each member keeps its own state and runs the device code it runs alone, so every output is
    bit for bit the stand-alone session's.  While grouped a member still takes ``reset()``,
    ``init_minmax_tracker()``, ``audio()`` and ``ongoing``; calling it with a hop raises.  ``close()`` gives the
    members back for stand-alone use (closing a member closes its group first).
    """

    def __init__(self, sessions):
        sessions = list(sessions)
        if not sessions:
            raise ValueError("HopSessionGroup: no sessions")
        for i, s in enumerate(sessions):
            if not isinstance(s, HopSession):
                raise TypeError(f"HopSessionGroup: member {i} is {type(s).__name__}, not a HopSession")
            if not s.handle:
                raise ValueError(f"HopSessionGroup: member {i} is closed")
            if any(s is t for t in sessions[:i]):
                raise ValueError(f"HopSessionGroup: member {i} is listed twice")
            if s._group is not None:
                raise ValueError(f"HopSessionGroup: member {i} already belongs to a group")
            if s._paired != sessions[0]._paired:  # all or none: the group's one kernel runs one kind of stage
                raise ValueError(f"HopSessionGroup: members 0 and {i} differ in having a voting locator "
                                 "(MultilateratePaired)")
        self._L = _lib.lib()
        self.handle = None
        n = len(sessions)
        members = (ctypes.c_void_p * n)(*[s.handle.value for s in sessions])
        h = ctypes.c_void_p()
        # (the library checks the rest -- hop in flight, graph form, device, n_fft, channels, locator, strength --
        #  on the host, before anything is launched)
        check(self._L.ofp_hop_group_create(members, n, ctypes.byref(h)), "ofp_hop_group_create")
        self.handle = h
        self.sessions = tuple(sessions)
        for s in sessions:
            s._group = self
        self._ptrs = (ctypes.c_void_p * n)()
        b, c = sessions[0].block_size, sessions[0].n_signals
        self._shape = (n, b, c) if all(s.block_size == b for s in sessions) else None  # hops as one [S, B, C] array
        self._collect = [(s, (s.handle, ctypes.byref(s._n), s._rec.ctypes.data,
                              s._logits.ctypes.data if s.n_out else None, s._mel.ctypes.data,
                              s._rel.ctypes.data if s.want_rel else None,
                              s._sg.ctypes.data if s.onset_strength else None)) for s in sessions]

    def __len__(self):
        return len(self.sessions)

    def close(self):
        if getattr(self, "handle", None):
            self._L.ofp_hop_group_destroy(self.handle)
            self.handle = None
            for s in self.sessions:
                s._group = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _fill(self, hops):
        """The members' hop pointers; the arrays they point into (kept alive by the caller of this method)."""
        if not self.handle:
            raise ValueError("HopSessionGroup: the group is closed")
        if isinstance(hops, np.ndarray) and hops.ndim == 3 and self._shape is not None:
            if hops.dtype != np.float32:  # (as HopSession._f32)
                raise ctypes.ArgumentError(f"array must have data type float32, got {hops.dtype}")
            if hops.shape != self._shape:
                raise ValueError(f"expected shape {self._shape}, got {hops.shape}")
            hops = np.ascontiguousarray(hops)
            base, step = hops.ctypes.data, hops[0].nbytes  # (not strides[0]: numpy leaves it free when S == 1)
            self._ptrs[:] = range(base, base + step * len(self.sessions), step)
            return hops
        if len(hops) != len(self.sessions):
            raise ValueError(f"expected {len(self.sessions)} hops, got {len(hops)}")
        keep = [s._f32(h, s.block_size) for s, h in zip(self.sessions, hops)]
        self._ptrs[:] = [h.ctypes.data for h in keep]
        return keep

    def submit(self, hops):
        """``hops``: ``[S, B, C]`` float32, or a sequence of S arrays ``[B_i, C]`` float32 (member i's hop)."""
        keep = self._fill(hops)
        check(self._L.ofp_hop_group_submit(self.handle, self._ptrs), "ofp_hop_group_submit")
        del keep  # (the library has copied the hops into the members' pinned buffers)

    def collect(self):
        """The members' result dicts, as ``HopSession.collect`` returns them."""
        check(self._L.ofp_hop_group_wait(self.handle), "ofp_hop_group_wait")
        return [s.collect() for s in self.sessions]

    def __call__(self, hops):
        self.submit(hops)
        return self.collect()

    def push_raw(self, hops):
        """`__call__` without building the result dicts (latency measurements): the S onset counts; the outputs stay
        in the members' host arrays."""
        self.submit(hops)
        L = self._L
        check(L.ofp_hop_group_wait(self.handle), "ofp_hop_group_wait")
        counts = []
        for s, a in self._collect:
            check(L.ofp_hop_collect(*a), "ofp_hop_collect")
            s.current_index += s.block_size
            counts.append(int(s._n.value))
        return counts
