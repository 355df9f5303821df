"""Hit location on MI355X -- drop-in surface of the reference's ``onset_fingerprinting/multilateration.py``.

Same names, arguments and returns as the reference for:
  * ``speed_of_sound`` and the coordinate transforms (host numpy: scalar formulas),
  * ``lag_map_2d`` / ``lag_map_3d`` (GPU, ``ofp_lag_maps``; numpy float32 back, bit-identical),
  * ``solve_trilateration`` / ``solve_trilateration_3d`` (GPU, ``ofp_trilaterate``: MINPACK hybrj as
    ``scipy.optimize.fsolve(..., fprime=jac, xtol=0.01, maxfev=20)`` runs it; a tuple, or None unless ier == 1),
  * ``Multilaterate3D``: lag maps and their extremes built by ``ofp_lag_maps``, ``is_legal_3d`` by
    ``ofp_locate_legal``, ``trilaterate`` by ``ofp_trilaterate`` (or the model's ``ofp_mlp_forward``), and
    ``locate`` -- the reference's host state machine, whose cross-correlation step runs on the device
    (``ofp_locate_section`` -> ``ofp_xcorr_lag`` -> ``ofp_adjust_onset``).

  * ``find_lag`` / ``find_lag_multi`` (GPU, ``ofp_find_lags``: np.correlate by the fp64 canon of ofp_xcorr_lag,
    np.argmax, scipy.signal.find_peaks and the top-n order; ties in that order by ascending lag, and a correlation
    with a non-finite value raises ValueError in ``find_lag_multi``),
  * ``Multilaterate``: the 2-D locator, its maps by ``ofp_lag_maps``, ``is_legal_3d`` by ``ofp_locate_legal``,
    ``trilaterate`` by ``ofp_trilaterate`` and ``locate`` the reference's host state machine,
  * ``MultilateratePaired``: the grid-voting locator.  Its neighbour maps are indexed once by lag value
    (``ofp_vote_index``); ``locate_cc`` correlates the windows (``ofp_find_lags``) and votes (``ofp_paired_vote``)
    by reading only the cells whose lag matches, and ``locate`` solves with ``ofp_trilaterate``.  2 <= S <= 16;
    ``locate_cc`` refuses onset_idx - left < 0 (the reference's slice would wrap),
  * ``lag_intensity_map`` (GPU: ``ofp_lag_maps`` and ``ofp_intensity_maps``) and its host helpers ``vec_sub``,
    ``attenuate_intensity``, ``sound_intensity_at_source``.

``Multilaterate3D.locate`` also exists as device code (csrc/ofp_locate_dev.h) on a device-resident copy of ``ongoing``:
``Multilaterate3D.locate_stream_device`` replays a stream of calls in one launch (``ofp_locate_stream``), and
``realtime.HopSession(locator=...)`` runs it inside the hop's graph.  The 2-D ``Multilaterate`` has the same three
device forms (the planar instantiation of the same ``loc_feed``; ``ofp_locate_stream_2d``, ``ofp_locate_groups_2d``,
``ofp_hop_set_locator_2d``).

Batched, device-resident additions: ``locate_groups_device`` locates every onset group ``group_onsets_device``
found, in one pass without host synchronisation; ``find_lags_device``, ``MultilateratePaired.locate_cc_device`` /
``locate_device`` and ``locate_cc_groups_device`` do the same for the 2-D functions.

There is no CPU path: every GPU function raises without the library or a gfx950 GPU.  Inputs to the correlations
are taken as float32.
"""
import ctypes
from typing import Optional

import numpy as np
import torch

from . import _lib, detection
from ._lib import check

TEMPERATURE = 20.0
HUMIDITY = 0.5
DIAMETER = 14 * 2.54
STRIKE_FORCE = 1.0
C_drumhead = 82  # m/s through a drumhead membrane
MEDIUM = "air"
ONSET_TOL = 50
NORM_CUTOFF = 10
lookaround = ONSET_TOL + NORM_CUTOFF
LOCATE_MAX_SECTION = 4096  # longest cross-correlation section of the device state machine (rows)

XTOL = 0.01  # solve_trilateration*'s fsolve arguments
MAXFEV = 20
# fsolve's info["nfev"] counts Python calls of the residual function: MINPACK's evaluations plus two of its own
# (a shape check and one call before the first Jacobian).  ofp_trilaterate reports MINPACK's count.
FSOLVE_EXTRA_CALLS = 2

LOCATE_UNUSED, LOCATE_FEW_CHANNELS, LOCATE_ILLEGAL_LAG, LOCATE_NO_CELL = -1, -2, -3, -4


# ---- host formulas ------------------------------------------------------------------------------------------

def speed_of_sound(scale: int = 1, temperature: float = TEMPERATURE, humidity: float = HUMIDITY,
                   medium=MEDIUM) -> float:
    """Speed of sound in m/s times `scale` (100: cm/s); 'air' depends on temperature and humidity, any other
    medium is the drumhead constant."""
    if medium != "air":
        return scale * C_drumhead
    return scale * (331.3 + 0.606 * temperature) * (1 + 0.0124 * humidity)


def _angle_deg(y, x):
    # arctan2 mapped to [0, 2 pi), in degrees
    return np.degrees(np.arctan2(y, x) % (2 * np.pi))


def cartesian_to_polar(x: float, y: float, r: float = None):
    """(x, y) -> (radius, angle in degrees in [0, 360)); the radius is divided by `r` when given."""
    rad = np.sqrt(x**2 + y**2)
    if r is not None:
        rad = rad / r
    return rad, _angle_deg(y, x)


def polar_to_cartesian(r: float, phi: float):
    """(radius, angle in degrees) -> (x, y)."""
    a = np.radians(phi)
    return r * np.cos(a), r * np.sin(a)


def spherical_to_cartesian(r: float, phi: float, theta: float):
    """(radius, x-y angle in degrees, elevation in degrees) -> (x, y, z).  A negative theta is taken as its
    magnitude measured from the z axis, otherwise theta is measured from the x-y plane."""
    p = np.radians(phi)
    t = np.radians(-theta if theta < 0 else 90 - theta)
    return r * np.cos(p) * np.sin(t), r * np.sin(p) * np.sin(t), r * np.cos(t)


def cartesian_to_spherical(x: float, y: float, z: float):
    """(x, y, z) -> (radius, x-y angle in degrees, elevation in degrees)."""
    rad = np.sqrt(x**2 + y**2 + z**2)
    phi = _angle_deg(y, x)
    theta = np.degrees(np.arccos(z / rad))
    return rad, phi, (-theta if theta < 0 else 90 - theta)


def cartesian_to_cylindrical(x: float, y: float, z: float, r: float = None):
    """(x, y, z) -> (radius, angle in degrees, z); the radius is divided by `r` when given."""
    rad, phi = cartesian_to_polar(x, y, r)
    return rad, phi, z


def cylindrical_to_cartesian(r: float, phi: float, z: float):
    """(radius, angle in degrees, z) -> (x, y, z)."""
    x, y = polar_to_cartesian(r, phi)
    return x, y, z


def remove_seed(groups, group):
    """The groups that do not start with `group`'s first (sensor, onset)."""
    seed = (group[0][0], group[1][0])
    return [g for g in groups if not (g[0][0] == seed[0] and g[1][0] == seed[1])]


# ---- device plumbing ----------------------------------------------------------------------------------------

def _dev(device):
    if isinstance(device, torch.device):
        return device
    return torch.device("cuda", int(device))


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _grid_3d(d, scale, tol):
    """lag_map_3d's grid: radius in cells and the squared mask radius."""
    r = int(np.round(d, 1) * scale) // 2
    return r, float((r + tol * scale) ** 2)


def _grid_2d(d, scale, tol):
    r = int(np.round(d * scale / 2))
    return r, float((r + tol * scale) ** 2)


def _sensor_array(sensors):
    s = np.array(sensors, dtype=np.float64)
    if s.ndim != 2 or s.shape[1] not in (2, 3):
        raise ValueError(f"sensor positions must be [S, 2] or [S, 3], got shape {s.shape}")
    if s.shape[1] == 2:
        s = np.concatenate([s, np.zeros((len(s), 1))], 1)
    if len(s) < 2:
        raise ValueError("need at least two sensors")
    return np.ascontiguousarray(s)


def lag_maps_device(sensors, r, c, sr, mask_r2, floor=None, device=0):
    """Lag maps of every ordered pair of `sensors` ([S, 3], cm): maps float32 [S, S, 2r+1, 2r+1] with
    maps[i, j] = lag_map_3d(sensors[j], sensors[i]) (NaN outside the circle, below `floor` and on i == j), and
    their nanmin / nanmax [S, S] (device tensors)."""
    s_np = _sensor_array(sensors)
    if int(r) < 0:
        raise ValueError(f"grid radius must be >= 0, got {r}")
    dev = _dev(device)
    s = torch.from_numpy(s_np).to(dev)
    S = s.shape[0]
    side = 2 * int(r) + 1
    maps = torch.empty((S, S, side, side), dtype=torch.float32, device=dev)
    mn = torch.empty((S, S), dtype=torch.float32, device=dev)
    mx = torch.empty((S, S), dtype=torch.float32, device=dev)
    check(_lib.lib().ofp_lag_maps(s.data_ptr(), S, int(r), float(c), float(sr), float(mask_r2),
                                  -np.inf if floor is None else float(floor), maps.data_ptr(), mn.data_ptr(),
                                  mx.data_ptr(), _stream(dev)), "ofp_lag_maps")
    return maps, mn, mx


def _one_map(mic_a, mic_b, r, c, sr, mask_r2, device):
    sensors = _sensor_array([list(mic_b) + [0.0] * (3 - len(mic_b)), list(mic_a) + [0.0] * (3 - len(mic_a))])
    dev = _dev(device)
    _lib.require_gpu(dev.index or 0)
    maps, _, _ = lag_maps_device(sensors, r, c, sr, mask_r2, device=dev)
    return maps[0, 1].cpu().numpy()


def lag_map_2d(mic_a, mic_b, d: int = DIAMETER, sr: int = 96000, scale: float = 1, medium: str = MEDIUM,
               tol: int = 1, c: Optional[float] = None, device=0):
    """multilateration.py:902-942: the lag (samples) from mic_b to mic_a over the drum's grid, float32."""
    if c is None:
        c = speed_of_sound(100 * scale, medium=medium)
    r, mask_r2 = _grid_2d(d, scale, tol)
    return _one_map(list(mic_a)[:2], list(mic_b)[:2], r, c, sr, mask_r2, device)


def lag_map_3d(mic_a, mic_b, d: int = DIAMETER, sr: int = 96000, scale: float = 1, medium: str = MEDIUM,
               tol: int = 1, c: Optional[float] = None, device=0):
    """multilateration.py:945-1001: lag_map_2d for microphones at (x, y, z) over the surface z = 0."""
    if c is None:
        c = speed_of_sound(100 * scale, medium=medium)
    r, mask_r2 = _grid_3d(d, scale, tol)
    return _one_map(list(mic_a), list(mic_b), r, c, sr, mask_r2, device)


def legal_cells_device(maps, sensors, onsets, tolerance):
    """is_legal_3d for G groups: maps float32 CUDA [S, S, side, side], sensors int32 [G, 3], onsets int64 [G, 3]
    -> int32 [G, 2] (col, row) of the first legal cell, (0, 0) if none."""
    assert maps.is_cuda and maps.dtype == torch.float32 and maps.is_contiguous() and maps.dim() == 4
    assert sensors.dtype == torch.int32 and onsets.dtype == torch.int64
    assert sensors.is_contiguous() and onsets.is_contiguous() and sensors.shape == onsets.shape
    S, side = maps.shape[0], maps.shape[2]
    G = sensors.shape[0]
    idx = torch.empty((G, 2), dtype=torch.int32, device=maps.device)
    check(_lib.lib().ofp_locate_legal(maps.data_ptr(), S, (side - 1) // 2, sensors.data_ptr(), onsets.data_ptr(), G,
                                      float(tolerance), idx.data_ptr(), _stream(maps.device)), "ofp_locate_legal")
    return idx


def trilaterate_device(geom, delta, guess, xtol=XTOL, maxfev=MAXFEV):
    """solve_trilateration_3d for G groups: geom float64 CUDA [G, 9] (origin, a, b as x, y, z), delta [G, 2],
    guess [G, 2] -> root float64 [G, 2], ier int32 [G] (1: converged), nfev int32 [G] (MINPACK's count)."""
    for t in (geom, delta, guess):
        assert t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()
    G = geom.shape[0]
    assert geom.shape == (G, 9) and delta.shape == (G, 2) and guess.shape == (G, 2)
    root = torch.empty((G, 2), dtype=torch.float64, device=geom.device)
    ier = torch.empty(G, dtype=torch.int32, device=geom.device)
    nfev = torch.empty(G, dtype=torch.int32, device=geom.device)
    check(_lib.lib().ofp_trilaterate(geom.data_ptr(), delta.data_ptr(), guess.data_ptr(), G, float(xtol), int(maxfev),
                                     root.data_ptr(), ier.data_ptr(), nfev.data_ptr(), _stream(geom.device)),
          "ofp_trilaterate")
    return root, ier, nfev


def _solve_one(a, b, o, dda, ddb, guess, device=0):
    geom_np = _sensor_array([o, a, b]).reshape(1, 9)
    x0_np = np.asarray(guess, dtype=np.float64).reshape(1, 2)
    dev = _dev(device)
    _lib.require_gpu(dev.index or 0)
    geom = torch.from_numpy(geom_np).to(dev)
    delta = torch.tensor([[float(dda), float(ddb)]], dtype=torch.float64, device=dev)
    root, ier, _ = trilaterate_device(geom, delta, torch.from_numpy(np.ascontiguousarray(x0_np)).to(dev))
    if int(ier.cpu()[0]) != 1:
        return None
    return tuple(np.float64(v) for v in root.cpu().numpy()[0])


def solve_trilateration(sensor_a, sensor_b, sensor_origin, delta_d_a: float, delta_d_b: float, initial_guess,
                        device=0):
    """multilateration.py:170-227 (2-D sensors): the point (x, y) or None."""
    return _solve_one(sensor_a, sensor_b, sensor_origin, delta_d_a, delta_d_b, initial_guess, device)


def solve_trilateration_3d(sensor_a, sensor_b, sensor_origin, delta_d_a: float, delta_d_b: float, initial_guess,
                           device=0):
    """multilateration.py:230-316 (3-D sensors, point on z = 0): the point (x, y) or None."""
    return _solve_one(sensor_a, sensor_b, sensor_origin, delta_d_a, delta_d_b, initial_guess, device)


def longest_section(max_max_lags, block_size: int) -> int:
    """max(max_max_lags) + block_size + lookaround + 1: the group's first onset lies at most max(max_max_lags)
    samples before the onset fed, which lies in the hop that ends at the counter."""
    return int(np.ceil(float(np.nanmax(max_max_lags)))) + int(block_size) + lookaround + 1


def check_locator_model(model, what):
    """ValueError unless `model` is None or a 2 -> 2 calibration.FCNN; host-side only (no GPU call)."""
    if model is None:
        return
    if not hasattr(model, "device_mlp"):
        raise ValueError(f"{what}: the model must be a calibration.FCNN (its ofp_mlp network)")
    lin = [m for m in model.modules() if isinstance(m, torch.nn.Linear)]
    if not lin or (lin[0].in_features, lin[-1].out_features) != (2, 2):
        got = f"{lin[0].in_features} -> {lin[-1].out_features}" if lin else "no"
        raise ValueError(f"{what}: the model maps {got} values, not 2 -> 2")


def ongoing_list(state):
    """A ``_lib.LocateState`` as the reference's ``ongoing``: a list of ([sensors], [onsets]).  Two entries that are
    one Python object in the reference (an extended group is appended twice) are one object here too."""
    out = []
    for g in range(state.n_groups):
        if state.alias[g] and out:
            out.append(out[-1])
            continue
        n = state.len[g]
        out.append(([int(v) for v in state.sensors[g][:n]], [int(v) for v in state.onsets[g][:n]]))
    return out


def check_locate_flags(flags, what):
    """The device state machine's sticky flags are never silent."""
    if flags & (_lib.LOCF_GROUPS | _lib.LOCF_MEMBERS):
        raise _lib.OnsetFPError(f"{what}: the locate state overflowed ({_lib.LOCS_GROUPS} groups of up to "
                                f"{_lib.LOCS_MEMBERS} members; flags {flags})")
    if flags & _lib.LOCF_SECTION:
        raise _lib.OnsetFPError(f"{what}: a cross-correlation section was longer than the bound or shorter than 3 rows "
                                f"(flags {flags})")
    if flags & _lib.LOCF_BAD_CALL:
        raise _lib.OnsetFPError(f"{what}: a call was refused (sensor index or counter out of range; flags {flags})")


# ---- what Multilaterate3D and Multilaterate share -------------------------------------------------------------

class _LagMapLocator:
    """The lag-map tables of a locator on its device, the two legality tests on them, and the device forms of
    ``locate``.  A subclass sets radius, sensor_locs, medium, sr and samples_per_cm, then calls ``_build_tables``."""

    def _speed(self):
        """The speed of sound in cm/s, as the class's ``trilaterate`` has it."""
        raise NotImplementedError

    def _build_tables(self, grid, drum_diameter, device):
        """The lag maps (1 cm grid, 2 cm tolerance at the edge, values below -samples_per_cm dropped) by
        ``ofp_lag_maps``, kept on `device`, and the reference's host views of them: ``lag_maps``, ``min_lags``,
        ``max_lags``, ``max_max_lags``.  grid: _grid_3d or _grid_2d.  Ends with an empty ``ongoing``."""
        sensors = _sensor_array(self.sensor_locs)  # [S, 3]; z = 0 for planar sensors
        self.device = _dev(device)
        _lib.require_gpu(self.device.index or 0)
        S = len(sensors)
        r, mask_r2 = grid(drum_diameter, 1, 2)
        self.grid_radius = r
        self.maps_dev, self.min_dev, self.max_dev = lag_maps_device(
            sensors, r, self._speed(), self.sr, mask_r2, floor=-self.samples_per_cm * 1, device=self.device)
        self.sensors_dev = torch.from_numpy(sensors).to(self.device)
        maps = self.maps_dev.cpu().numpy()
        mn, mx = self.min_dev.cpu().numpy(), self.max_dev.cpu().numpy()
        self.lag_maps = [{j: maps[i, j] for j in range(S) if j != i} for i in range(S)]
        self.max_lags = [{j: mx[i, j] for j in range(S) if j != i} for i in range(S)]
        self.min_lags = [{j: mn[i, j] for j in range(S) if j != i} for i in range(S)]
        self.max_max_lags = [np.nanmax(list(d.values())) for d in self.max_lags]
        self.ongoing = []

    def is_legal(self, first_sensor: int, later_sensor: int, lag: int) -> bool:
        """The lag lies strictly between the extremes of the pair's lag map."""
        return self.min_lags[first_sensor][later_sensor] < lag < self.max_lags[first_sensor][later_sensor]

    def is_legal_3d(self, group, tolerance=1):
        """multilateration.py:413-426 and :663-676: (col, row) of the first map cell consistent with both lags of the
        group within `tolerance` cm, (0, 0) when there is none."""
        sensors, onsets = group[0], group[1]
        s = torch.tensor([[int(v) for v in sensors[:3]]], dtype=torch.int32, device=self.device)
        o = torch.tensor([[int(v) for v in onsets[:3]]], dtype=torch.int64, device=self.device)
        idx = legal_cells_device(self.maps_dev, s, o, tolerance * self.samples_per_cm).cpu().numpy()[0]
        return int(idx[0]), int(idx[1])

    def _locator_struct(self, xtol, maxfev, use_audio=0, max_section=0, mlp=None):
        """The ofp_hop_locator of this object's device tables (they must outlive every call that uses it)."""
        loc = _lib.HopLocator()
        loc.d_sensors, loc.S = self.sensors_dev.data_ptr(), self.sensors_dev.shape[0]
        loc.d_maps, loc.d_min, loc.d_max = self.maps_dev.data_ptr(), self.min_dev.data_ptr(), self.max_dev.data_ptr()
        loc.r = self.grid_radius
        loc.samples_per_cm, loc.sr, loc.c, loc.radius = float(self.samples_per_cm), float(self.sr), \
            float(self._speed()), float(self.radius)
        loc.xtol, loc.maxfev = float(xtol), int(maxfev)
        loc.mlp = mlp.handle if mlp is not None else None
        loc.use_audio, loc.max_section = int(bool(use_audio)), int(max_section)
        return loc

    def _replay(self, entry, loc, columns, recording=()):
        """One launch of a stream entry point (`entry`: its name) with the ofp_hop_locator `loc`, from an empty state.
        columns: the per-call arrays by name -- sensors first, int32; the others int64 -- in the entry point's order;
        recording: what it takes between the call count and the state.  Returns (found bool [K], xy float64 [K, 2]
        with NaN where nothing was returned, ongoing as ``ongoing_list`` gives it); the sticky flags raise."""
        cols = [np.ascontiguousarray(a, dtype=np.int64 if k else np.int32).reshape(-1)
                for k, a in enumerate(columns.values())]
        K = len(cols[0])
        if any(len(a) != K for a in cols):
            raise ValueError("locate_stream_device: " + ", ".join(f"{len(a)} {n}" for a, n in zip(cols, columns)))
        dev = self.device
        cols = [torch.from_numpy(a).to(dev) for a in cols]
        state = torch.zeros(ctypes.sizeof(_lib.LocateState), dtype=torch.uint8, device=dev)
        found = torch.zeros(max(K, 1), dtype=torch.int32, device=dev)
        xy = torch.full((max(K, 1), 2), float("nan"), dtype=torch.float64, device=dev)
        check(getattr(_lib.lib(), entry)(ctypes.byref(loc), *(a.data_ptr() for a in cols), K, *recording,
                                         state.data_ptr(), found.data_ptr(), xy.data_ptr(), _stream(dev)), entry)
        st = _lib.LocateState.from_buffer_copy(state.cpu().numpy().tobytes())
        check_locate_flags(st.flags, "locate_stream_device")
        return found.cpu().numpy()[:K].astype(bool), xy.cpu().numpy()[:K], ongoing_list(st)


# ---- Multilaterate3D ----------------------------------------------------------------------------------------

class Multilaterate3D(_LagMapLocator):
    def __init__(self, sensor_locations, drum_diameter: float = DIAMETER, medium: str = "drumhead", sr: int = 44100,
                 c: Optional[float] = None, model=None, device=0):
        """multilateration.py:320-387.  sensor_locations: (relative radius, angle, elevation) per sensor; c in m/s
        (speed_of_sound when None); model: a calibration.FCNN that replaces the solver.  The lag maps (1 cm grid,
        2 cm tolerance at the edge, values below -samples_per_cm dropped) stay on `device`; ``lag_maps``,
        ``min_lags``, ``max_lags``, ``max_max_lags`` are the reference's host views of them."""
        self.c = speed_of_sound(100, medium=medium) if c is None else c * 100
        self.model = model
        if model is not None:
            self.model.eval()
        self.radius = drum_diameter / 2
        self.sensor_locs = [spherical_to_cartesian(x[0] * self.radius, x[1], x[2]) for x in sensor_locations]
        self.medium = medium
        self.sr = sr
        self.samples_per_cm = sr / self.c
        self._build_tables(_grid_3d, drum_diameter, device)

    def _speed(self):
        return self.c

    def trilaterate(self, group, initial_guess):
        """multilateration.py:536-565 (reorders `group` in place when its second sensor is sensor 1)."""
        sensors, onsets = group[0], group[1]
        if sensors[1] == 1:
            sensors[1:] = [0, 1]
            onsets[1:] = onsets[2:0:-1]
        d_a1 = onsets[1] - onsets[0]
        d_b1 = onsets[2] - onsets[0]
        if self.model is not None:  # cm, hence * 100
            return self.model.call_np((d_a1, d_b1)) * 100
        return solve_trilateration_3d(self.sensor_locs[sensors[1]], self.sensor_locs[sensors[2]],
                                      self.sensor_locs[sensors[0]], d_a1 / self.sr * self.c,
                                      d_b1 / self.sr * self.c, initial_guess, device=self.device)

    def _cc_adjust(self, group, sensor_index, onset_index, rec_audio):
        """locate's cross-correlation refinement (multilateration.py:452-497) on the device: returns (lag or None,
        move of the group's first onset, move of the new onset)."""
        last_onset = group[1][0]
        i = rec_audio.counter - last_onset + lookaround
        sec = rec_audio[-i - 1:]
        sec = sec if torch.is_tensor(sec) else torch.from_numpy(np.ascontiguousarray(sec))
        sec = sec.to(self.device, torch.float32).contiguous()
        n, C = sec.shape
        out = torch.empty((2, max(n - 1, 1)), dtype=torch.float32, device=self.device)
        check(_lib.lib().ofp_locate_section(sec.data_ptr(), n, C, int(group[0][0]), int(sensor_index),
                                            out.data_ptr(), _stream(self.device)), "ofp_locate_section")
        m = n - 1
        current = onset_index - group[1][0]
        lo, hi = detection._py_slice(m - current - ONSET_TOL, m - current + ONSET_TOL, 2 * m - 1)
        if hi <= lo:
            return None, 0, 0
        i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=self.device)
        x, y = out[0:1], out[1:2]
        am = int(detection.xcorr_lags_device(x, y, i32([lo]), i32([hi]), 0, False, NORM_CUTOFF).cpu()[0])
        new_lag = -(am - (current + ONSET_TOL))
        og = [lookaround, onset_index - last_onset + lookaround]
        mv = detection.adjust_onsets_device(x, y, i32([og]), i32([new_lag])).cpu().numpy()[0]
        return new_lag, int(mv[0]), int(mv[1])

    def locate(self, sensor_index: int, onset_index: int, rec_audio=None):
        """multilateration.py:428-534: feed one onset; returns the location of the hit it completes, or None.
        rec_audio: the recording ring (``.counter`` = samples written, ``[-k:]`` = the last k rows [k, C])."""
        new_groups = []
        for group in self.ongoing:
            # group: ([sensor indices], [onset indices]); lags are measured from the group's first onset
            lag = onset_index - group[1][0]
            if lag > self.max_max_lags[group[0][0]]:
                continue
            if lag < 0:  # an adjustment moved an onset behind this one: swap them
                first = (group[0][0], group[1][0])
                group[0][0], group[1][0] = sensor_index, onset_index
                sensor_index, onset_index = first
                lag = -lag
            if sensor_index not in group[0]:
                if rec_audio is not None:
                    new_lag, co, cn = self._cc_adjust(group, sensor_index, onset_index, rec_audio)
                    if new_lag is not None:
                        lag = new_lag
                        group[1][0] += co
                        onset_index += cn
                if self.is_legal(group[0][0], sensor_index, lag):
                    group = (group[0] + [sensor_index], group[1] + [onset_index])
                    if len(group[0]) == 3:
                        if group[0][0] == group[0][1]:
                            break
                        res = self.is_legal_3d(group)
                        if res != (0, 0):
                            res = self.trilaterate(group, initial_guess=np.array(res) - self.radius)
                            if res is not None:
                                new_groups = remove_seed(new_groups, group)
                            self.ongoing = new_groups
                            return res
                    new_groups.append(group)
            if lag <= self.max_max_lags[group[0][0]]:
                new_groups.append(group)
        new_groups.append(([sensor_index], [onset_index]))
        self.ongoing = new_groups
        return None

    # ---- locate on the device ------------------------------------------------------------------------------

    def _device_model(self, what):
        """The model's ofp_mlp network (None without a model); ValueError unless it is a 2 -> 2 calibration.FCNN."""
        check_locator_model(self.model, what)
        return self.model.device_mlp(self.device) if self.model is not None else None

    def locator_struct(self, use_audio, max_section, mlp=None, xtol=XTOL, maxfev=MAXFEV):
        """The ofp_hop_locator of this object's device tables (they must outlive every call that uses it)."""
        return self._locator_struct(xtol, maxfev, use_audio, max_section, mlp)

    def locate_stream_device(self, sensors, onsets, counters, audio=None):
        """``locate`` for a whole stream of calls in ONE launch (``ofp_locate_stream``): call k feeds
        (sensors[k], onsets[k]) with a ring that holds ``audio[:counters[k]]`` (audio [N, C] float32, numpy or a
        CUDA tensor; None: no cross-correlation step).  Starts from an empty state and does not touch
        ``self.ongoing``.  Returns (found bool [K], xy float64 [K, 2] with NaN where nothing was returned, ongoing:
        the final state as the reference's list of ([sensors], [onsets])).  Raises OnsetFPError when the state
        overflowed (64 groups of 8 members), a section was longer than LOCATE_MAX_SECTION rows, or a call was refused
        (the kernel checks every call: sensor outside 0..S-1, counter outside the recording)."""
        S = self.sensors_dev.shape[0]
        mlp = self._device_model("locate_stream_device")
        ad, n_rows, n_ch, max_section = None, 0, 0, 0
        if audio is not None:
            ad = audio if torch.is_tensor(audio) else torch.from_numpy(np.ascontiguousarray(audio, dtype=np.float32))
            if ad.dim() != 2 or ad.shape[1] < S:
                raise ValueError(f"locate_stream_device: audio must be [N, C >= {S}], got {tuple(ad.shape)}")
            ad = ad.to(self.device, torch.float32).contiguous()
            n_rows, n_ch = ad.shape
            max_section = LOCATE_MAX_SECTION  # the counters are the caller's: any section the kernel can hold
        loc = self.locator_struct(audio is not None, max_section, mlp)
        return self._replay("ofp_locate_stream", loc, dict(sensors=sensors, onsets=onsets, counters=counters),
                            (_ptr(ad), n_rows, n_ch))


# ---- batched offline locator --------------------------------------------------------------------------------

def locate_groups_device(groups, n_groups, m, xtol=XTOL, maxfev=MAXFEV, return_guess=False):
    """Locate every onset group of a batch on the device, without host synchronisation.

    groups int64 CUDA [n_clips, cap_groups, C] and n_groups int64 [n_clips] (or None: every row), as
    `detection.group_onsets_device` returns them (optionally after `detection.fix_onsets_device`); channel k is
    sensor k of `m` (C <= number of sensors).  Per row, the reference's own steps in the order
    ``Multilaterate3D.locate`` applies them: the three earliest channels present, ordered by onset (ties by channel
    index), are origin, a and b; ``is_legal(origin, a)`` and ``is_legal(origin, b)``; ``is_legal_3d``;
    ``trilaterate`` from the guess (col, row) - radius, with its reordering (or ``m.model``).

    `m` may also be a 2-D ``Multilaterate`` (``ofp_locate_groups_2d``): the same row rule and status codes, with that
    class's ``trilaterate`` -- no reordering, deltas lag * c / sr, no model.  xy is then the Cartesian root in cm,
    and ``cartesian_to_polar(x, y, m.radius)`` gives the reference's tuple.

    Returns xy float64 [n_clips, cap_groups, 2] (NaN where no solve ran) and status int32 [n_clips, cap_groups]:
    fsolve's ier (1 = located; the reference drops every other value), or LOCATE_UNUSED (-1, row beyond the clip's
    groups), LOCATE_FEW_CHANNELS (-2), LOCATE_ILLEGAL_LAG (-3), LOCATE_NO_CELL (-4).  With return_guess, also the
    initial guesses [n_clips, cap_groups, 2] (NaN where none was formed)."""
    if not (torch.is_tensor(groups) and groups.is_cuda and groups.dtype == torch.int64 and groups.dim() == 3):
        raise ValueError("locate_groups_device: groups must be an int64 CUDA tensor [n_clips, cap_groups, C]")
    groups = groups.contiguous()
    n_clips, cap, C = groups.shape
    if C > m.sensors_dev.shape[0]:
        raise ValueError(f"locate_groups_device: {C} channels but {m.sensors_dev.shape[0]} sensors")
    if n_groups is not None and (n_groups.dtype != torch.int64 or n_groups.shape != (n_clips,) or not n_groups.is_cuda):
        raise ValueError("locate_groups_device: n_groups must be an int64 CUDA tensor [n_clips]")
    dev = groups.device
    mlp = None
    planar = isinstance(m, Multilaterate)
    if not planar and m.model is not None:
        if not hasattr(m.model, "device_mlp"):
            raise TypeError("locate_groups_device: the model must be a calibration.FCNN (its ofp_mlp network)")
        mlp = m.model.device_mlp(dev)
        if (mlp.n_in, mlp.n_out) != (2, 2):
            raise ValueError(f"locate_groups_device: the model maps {mlp.n_in} -> {mlp.n_out} values, not 2 -> 2")
        if not mlp.fits:
            raise ValueError("locate_groups_device: the model is too large for one ofp_mlp_forward launch")
    L = _lib.lib()
    rows = n_clips * cap
    xy = torch.empty((n_clips, cap, 2), dtype=torch.float64, device=dev)
    status = torch.empty((n_clips, cap), dtype=torch.int32, device=dev)
    guess = torch.empty((n_clips, cap, 2), dtype=torch.float64, device=dev) if return_guess else None
    ws = torch.empty(max(int(L.ofp_locate_workspace_bytes(rows)), 16), dtype=torch.uint8, device=dev)
    entry, net = "ofp_locate_groups", (mlp.handle if mlp is not None else None,)
    if planar:  # the same arguments without the network
        entry, net = "ofp_locate_groups_2d", ()
    check(getattr(L, entry)(groups.data_ptr(), n_clips, cap, C, _ptr(n_groups), m.sensors_dev.data_ptr(),
                            m.sensors_dev.shape[0], m.maps_dev.data_ptr(), m.min_dev.data_ptr(), m.max_dev.data_ptr(),
                            m.grid_radius, float(m.samples_per_cm), float(m.sr), float(m._speed()), float(m.radius),
                            float(xtol), int(maxfev), *net, xy.data_ptr(), status.data_ptr(), _ptr(guess),
                            ws.data_ptr(), ws.numel(), _stream(dev)), entry)
    return (xy, status, guess) if return_guess else (xy, status)


# ---- find_lag / find_lag_multi ------------------------------------------------------------------------------

FIND_LAG_MAX_LEN = 4096  # longest row ofp_find_lags correlates
FIND_LAG_MAX_TOP = 16    # most peaks it reports


def find_lags_device(a, b, top_n: int = 0, len_a=None, len_b=None):
    """find_lag / find_lag_multi for every row pair of float32 CUDA tensors a [n, La], b [n, Lb] (ofp_find_lags).

    len_a / len_b: optional int32 CUDA [n] row lengths (1..La / 1..Lb), the full rows otherwise.  Returns CUDA
    tensors lag int32 [n] (np.argmax of np.correlate(a, b, "full") - (len_a - 1)), peak_lag int32 [n, top_n],
    peak_val float32 [n, top_n] (cc ** 2; NaN in unused slots) and n_peaks int32 [n]: the slots used (0 when
    top_n == 0), -1 for a row
    whose correlation holds a non-finite value (no peaks reported), -2 for a row of length 0."""
    for name, t in (("a", a), ("b", b)):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2):
            raise ValueError(f"find_lags_device: {name} must be a float32 CUDA tensor [n, L]")
    if a.shape[0] != b.shape[0]:
        raise ValueError(f"find_lags_device: {a.shape[0]} rows of a but {b.shape[0]} of b")
    n, La = a.shape
    Lb = b.shape[1]
    if not (1 <= La <= FIND_LAG_MAX_LEN and 1 <= Lb <= FIND_LAG_MAX_LEN):
        raise ValueError(f"find_lags_device: row lengths {La}, {Lb} outside 1..{FIND_LAG_MAX_LEN}")
    if not 0 <= int(top_n) <= FIND_LAG_MAX_TOP:
        raise ValueError(f"find_lags_device: top_n {top_n} outside 0..{FIND_LAG_MAX_TOP}")
    for name, t in (("len_a", len_a), ("len_b", len_b)):
        if t is not None and not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.int32 and t.shape == (n,)):
            raise ValueError(f"find_lags_device: {name} must be an int32 CUDA tensor [{n}]")
    a, b = a.contiguous(), b.contiguous()
    len_a = len_a.contiguous() if len_a is not None else None
    len_b = len_b.contiguous() if len_b is not None else None
    dev = a.device
    top_n = int(top_n)
    lag = torch.empty(n, dtype=torch.int32, device=dev)
    peak_lag = torch.empty((n, top_n), dtype=torch.int32, device=dev)
    peak_val = torch.empty((n, top_n), dtype=torch.float32, device=dev)
    n_peaks = torch.empty(n, dtype=torch.int32, device=dev)
    check(_lib.lib().ofp_find_lags(a.data_ptr(), b.data_ptr(), n, La, Lb, 1, None, None, La, Lb, _ptr(len_a),
                                   _ptr(len_b), top_n, lag.data_ptr(), _ptr(peak_lag) if top_n else None,
                                   _ptr(peak_val) if top_n else None, n_peaks.data_ptr(), _stream(dev)),
          "ofp_find_lags")
    return lag, peak_lag, peak_val, n_peaks


def _pair_rows(a, b, device):
    a = np.asarray(a, dtype=np.float32).reshape(-1)
    b = np.asarray(b, dtype=np.float32).reshape(-1)
    if a.size == 0 or b.size == 0:
        raise ValueError("find_lag: a and b must not be empty")  # as np.correlate
    if a.size > FIND_LAG_MAX_LEN or b.size > FIND_LAG_MAX_LEN:
        raise ValueError(f"find_lag: rows of {a.size} and {b.size} samples; at most {FIND_LAG_MAX_LEN}")
    dev = _dev(device)
    _lib.require_gpu(dev.index or 0)
    return torch.from_numpy(a).to(dev).reshape(1, -1), torch.from_numpy(b).to(dev).reshape(1, -1)


def find_lag(a, b, device=0) -> int:
    """multilateration.py:878-887: np.argmax(np.correlate(a, b, "full")) - (len(a) - 1), on float32 copies."""
    ta, tb = _pair_rows(a, b, device)
    lag, _, _, _ = find_lags_device(ta, tb)
    return int(lag.cpu()[0])


def find_lag_multi(a, b, top_n: int = 3, device=0):
    """multilateration.py:890-899: the top_n peaks of scipy.signal.find_peaks over np.correlate(a, b, "full") by
    descending value, as (lags int64, cc ** 2 float32).  Exact ties are ordered by ascending lag (numpy's argsort
    leaves their order undefined).  A correlation with a non-finite value raises ValueError."""
    if not 0 <= int(top_n) <= FIND_LAG_MAX_TOP:
        raise ValueError(f"find_lag_multi: top_n {top_n} outside 0..{FIND_LAG_MAX_TOP}")
    ta, tb = _pair_rows(a, b, device)
    if int(top_n) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.float32)
    _, pl, pv, npk = find_lags_device(ta, tb, top_n)
    k = int(npk.cpu()[0])
    if k < 0:
        raise ValueError("find_lag_multi: the correlation holds a non-finite value")
    return pl.cpu().numpy()[0, :k].astype(np.int64), pv.cpu().numpy()[0, :k]


# ---- Multilaterate (2-D) ------------------------------------------------------------------------------------

class Multilaterate(_LagMapLocator):
    def __init__(self, sensor_locations, drum_diameter: float = DIAMETER, medium: str = "drumhead", sr: int = 44100,
                 device=0):
        """multilateration.py:578-645.  sensor_locations: (relative radius, angle) per sensor.  The lag maps (1 cm
        grid, 2 cm tolerance at the edge, values below -samples_per_cm dropped) are built by ``ofp_lag_maps`` and
        stay on `device`; ``lag_maps``, ``min_lags``, ``max_lags``, ``max_max_lags`` are the reference's host
        views of them."""
        self.radius = drum_diameter / 2
        self.sensor_locs = [polar_to_cartesian(x[0] * self.radius, x[1]) for x in sensor_locations]
        self.medium = medium
        self.sr = sr
        self.samples_per_cm = sr / speed_of_sound(100, medium=medium)
        self._build_tables(_grid_2d, drum_diameter, device)

    def _speed(self):
        return speed_of_sound(100, medium=self.medium)

    def locate(self, sensor_index: int, onset_index: int):
        """multilateration.py:678-711: feed one onset; returns (radius / drum radius, angle) of the hit it
        completes, or None.  Kept as the reference has it: a group that passes is_legal is appended twice, and the
        guess is (col, row) - radius on the grid of radius round(radius)."""
        new_groups = []
        for group in self.ongoing:
            lag = onset_index - group[1][0]
            if sensor_index not in group[0]:
                if self.is_legal(group[0][0], sensor_index, lag):
                    group = (group[0] + [sensor_index], group[1] + [onset_index])
                    if len(group[0]) == 3:
                        res = self.is_legal_3d(group)
                        if res != (0, 0):
                            res = self.trilaterate(group, np.array(res) - self.radius)
                            self.ongoing = new_groups
                            return res
                    new_groups.append(group)
            if lag <= self.max_max_lags[group[0][0]]:
                new_groups.append(group)
        new_groups.append(([sensor_index], [onset_index]))
        self.ongoing = new_groups
        return None

    def trilaterate(self, group, initial_guess):
        """multilateration.py:713-733: solve_trilateration (``ofp_trilaterate``) -> cartesian_to_polar(x, y,
        radius), or None.  No sensor reordering."""
        sensors, onsets = group[0], group[1]
        c = speed_of_sound(100, medium=self.medium)
        d_a1 = (onsets[1] - onsets[0]) * c / self.sr
        d_b1 = (onsets[2] - onsets[0]) * c / self.sr
        res = solve_trilateration(self.sensor_locs[sensors[1]], self.sensor_locs[sensors[2]],
                                  self.sensor_locs[sensors[0]], d_a1, d_b1, initial_guess, device=self.device)
        if res is None:
            return None
        return cartesian_to_polar(*res, self.radius)

    # ---- locate on the device ------------------------------------------------------------------------------

    def locator_struct(self, xtol=XTOL, maxfev=MAXFEV):
        """The ofp_hop_locator of this object's device tables (they must outlive every call that uses it), for the
        planar entry points: no cross-correlation step (use_audio 0, max_section 0) and no network."""
        return self._locator_struct(xtol, maxfev)

    def locate_stream_device(self, sensors, onsets):
        """``locate`` for a whole stream of calls in ONE launch (``ofp_locate_stream_2d``): call k feeds
        (sensors[k], onsets[k]).  Starts from an empty state and does not touch ``self.ongoing``.  Returns (found
        bool [K], rphi float64 [K, 2]: (radius / drum radius, angle) as ``locate`` returns it, NaN where nothing was
        returned, ongoing: the final state as the reference's list of ([sensors], [onsets])).  The device returns the
        Cartesian root; ``cartesian_to_polar`` is applied here, on the host, as ``trilaterate`` applies it.  Raises
        OnsetFPError when the state overflowed (64 groups of 8 members) or a call was refused (sensor outside
        0..S-1)."""
        found, xy, ongoing = self._replay("ofp_locate_stream_2d", self.locator_struct(),
                                          dict(sensors=sensors, onsets=onsets))
        rphi = np.full((len(found), 2), np.nan, dtype=np.float64)
        for k in np.flatnonzero(found):
            rphi[k] = cartesian_to_polar(np.float64(xy[k, 0]), np.float64(xy[k, 1]), self.radius)
        return found, rphi, ongoing


# ---- MultilateratePaired ------------------------------------------------------------------------------------

PAIRED_OK, PAIRED_UNUSED, PAIRED_NO_CHANNEL = 0, -1, -2
PAIRED_NEG_WINDOW, PAIRED_EMPTY_WINDOW, PAIRED_BAD_HIT = -5, -6, -7
PAIRED_MAX_SENSORS = 16  # all S x S maps of ofp_lag_maps stay on the device: 16 x 16 x 0.5 MB at scale 10


class MultilateratePaired:
    def __init__(self, sensor_locations, drum_diameter: float = DIAMETER, scale: float = 10,
                 medium: str = "drumhead", sr: int = 44100, device=0):
        """multilateration.py:736-796.  The neighbour maps lag_map_2d(s_i, s_j, scale=scale, medium="drumhead")
        for j = (i - 1) % S, (i + 1) % S are built by ``ofp_lag_maps`` and indexed once by ``ofp_vote_index``;
        ``lag_maps`` (list of dicts) and ``res`` are the reference's host views.  2 <= S <= 16."""
        S = len(sensor_locations)
        if not 2 <= S <= PAIRED_MAX_SENSORS:
            raise ValueError(f"MultilateratePaired: {S} sensors; 2..{PAIRED_MAX_SENSORS} supported")
        self.radius = int(np.round(drum_diameter * scale / 2, 1))
        self.sensor_locs = [polar_to_cartesian(x[0] * self.radius, x[1]) for x in sensor_locations]
        self.scale = scale
        self.medium = medium
        self.sr = sr
        self.device = _dev(device)
        _lib.require_gpu(self.device.index or 0)
        sensors = _sensor_array(self.sensor_locs)
        r, mask_r2 = _grid_2d(drum_diameter, scale, 1)
        self.side = 2 * r + 1
        self.maps_dev, mn, mx = lag_maps_device(sensors, r, speed_of_sound(100 * scale, medium="drumhead"), sr,
                                                mask_r2, device=self.device)
        self.sensors_dev = torch.from_numpy(sensors).to(self.device)
        # the reference's map (i, j) = lag_map_2d(s_i, s_j) is ofp_lag_maps' map (j, i); slot 2i + k of the index
        # holds sensor i's neighbour (i - 1) % S (k = 0) and (i + 1) % S (k = 1)
        self.neighbours = [((i - 1) % S, (i + 1) % S) for i in range(S)]
        ids = [j * S + i for i in range(S) for j in self.neighbours[i]]
        mn, mx = mn.cpu().numpy().reshape(-1)[ids], mx.cpu().numpy().reshape(-1)[ids]
        empty = np.isnan(mn)
        vmin = np.where(empty, 0, mn).astype(np.int64)
        vmax = np.where(empty, 0, mx).astype(np.int64)
        self.n_buckets = int((vmax - vmin).max()) + 1
        cells = self.side * self.side
        dev = self.device
        self.map_ids = torch.tensor(ids, dtype=torch.int32, device=dev)
        self.vmin = torch.from_numpy(vmin.astype(np.int32)).to(dev)
        self.starts = torch.empty((2 * S, self.n_buckets + 1), dtype=torch.int32, device=dev)
        self.sorted_cells = torch.empty((2 * S, cells), dtype=torch.int32, device=dev)
        bad = torch.empty(2 * S, dtype=torch.int32, device=dev)
        check(_lib.lib().ofp_vote_index(self.maps_dev.data_ptr(), cells, self.map_ids.data_ptr(), 2 * S,
                                        self.vmin.data_ptr(), self.n_buckets, self.starts.data_ptr(),
                                        self.sorted_cells.data_ptr(), bad.data_ptr(), _stream(dev)), "ofp_vote_index")
        if int(bad.sum().cpu()) != 0:
            raise RuntimeError("MultilateratePaired: a lag map holds a non-integer value; the vote index needs "
                               "integer maps")
        maps = self.maps_dev.cpu().numpy()
        self.lag_maps = [{j: maps[j, i] for j in self.neighbours[i]} for i in range(S)]
        self.res = np.zeros_like(self.lag_maps[0][1])

    def _c(self):
        return speed_of_sound(100 * self.scale, medium=self.medium)

    def locate(self, lags, i: int):
        """multilateration.py:798-834: (radius / self.radius, angle) from the lags to the neighbours of sensor i;
        raises TypeError where the reference does (a failed solve)."""
        S = len(self.sensor_locs)
        js = [(i - 1) % S, (i + 1) % S]
        sensor_a, sensor_b, sensor_origin = self.sensor_locs[js[0]], self.sensor_locs[js[1]], self.sensor_locs[i]
        c = self._c()
        d_a1 = lags[0] * c / self.sr
        d_b1 = lags[1] * c / self.sr
        weight_a = abs(d_a1) / self.radius
        weight_b = abs(d_b1) / self.radius
        weight_o = abs(d_a1 + d_b1) / (2 * self.radius)
        guess = np.array([sensor_a[0] * weight_a + sensor_b[0] * weight_b + sensor_origin[0] * weight_o,
                          sensor_a[1] * weight_a + sensor_b[1] * weight_b + sensor_origin[1] * weight_o])
        x, y = solve_trilateration(sensor_a, sensor_b, sensor_origin, d_a1, d_b1, guess, device=self.device)
        return cartesian_to_polar(x, y, self.radius)

    def locate_device(self, lags, first, xtol=XTOL, maxfev=MAXFEV):
        """``locate`` for B rows at once (``ofp_paired_solve``): lags int32 CUDA [B, 2], first int32 [B] ->
        rphi float64 [B, 2] (the polar result of the last iterate) and ier int32 [B] (1: the reference returns;
        any other value: it raises)."""
        if not (torch.is_tensor(lags) and lags.is_cuda and lags.dtype == torch.int32 and lags.dim() == 2
                and lags.shape[1] == 2):
            raise ValueError("locate_device: lags must be an int32 CUDA tensor [B, 2]")
        B = lags.shape[0]
        if not (torch.is_tensor(first) and first.dtype == torch.int32 and first.shape == (B,) and first.is_cuda):
            raise ValueError(f"locate_device: first must be an int32 CUDA tensor [{B}]")
        lags, first = lags.contiguous(), first.contiguous()
        dev = lags.device
        root = torch.empty((B, 2), dtype=torch.float64, device=dev)
        rphi = torch.empty((B, 2), dtype=torch.float64, device=dev)
        ier = torch.empty(B, dtype=torch.int32, device=dev)
        check(_lib.lib().ofp_paired_solve(self.sensors_dev.data_ptr(), self.sensors_dev.shape[0], lags.data_ptr(),
                                          first.data_ptr(), B, float(self._c()), float(self.sr), float(self.radius),
                                          float(xtol), int(maxfev), root.data_ptr(), rphi.data_ptr(), ier.data_ptr(),
                                          _stream(dev)), "ofp_paired_solve")
        return rphi, ier

    def _vote(self, x, hits, groups, tol, left, right, want_res=False):
        """x float32 CUDA [n_clips, N, C]; hits = (onset int64 [B], first int32 [B], clip int32 [B] or None) or
        groups = (groups int64 [n_clips, cap, C], n_groups or None) -> rphi, cell, status, lags (and res)."""
        S = len(self.sensor_locs)
        n_clips, N, C = x.shape
        if C < S:
            raise ValueError(f"locate_cc: {C} channels but {S} sensors")
        if not (0 <= int(left) and int(right) >= 1 and int(left) + int(right) <= FIND_LAG_MAX_LEN):
            raise ValueError(f"locate_cc: left {left}, right {right}: need left >= 0, right >= 1 and a window of at "
                             f"most {FIND_LAG_MAX_LEN} samples")
        if float(tol) < 0:
            raise ValueError(f"locate_cc: tol {tol} < 0")
        dev = x.device
        L = _lib.lib()
        if groups is not None:
            g, n_groups = groups
            cap = g.shape[1]
            B = n_clips * cap
            onset = first = clip = None
        else:
            onset, first, clip = hits
            B = onset.shape[0]
            g, n_groups, cap = None, None, 0
        i64 = lambda n_: torch.empty(n_, dtype=torch.int64, device=dev)
        i32 = lambda n_: torch.empty(n_, dtype=torch.int32, device=dev)
        a_off, b_off, ln, first_out, st_in = i64(2 * B), i64(2 * B), i32(2 * B), i32(B), i32(B)
        check(L.ofp_paired_windows(n_clips, N, C, S, _ptr(onset), _ptr(first), _ptr(clip), _ptr(g), cap,
                                   _ptr(n_groups), B, int(left), int(right), a_off.data_ptr(), b_off.data_ptr(),
                                   ln.data_ptr(), first_out.data_ptr(), st_in.data_ptr(), _stream(dev)),
              "ofp_paired_windows")
        w = int(left) + int(right)
        lags = i32(2 * B)
        if B:
            check(L.ofp_find_lags(x.data_ptr(), x.data_ptr(), 2 * B, 0, 0, C, a_off.data_ptr(), b_off.data_ptr(), w, w,
                                  ln.data_ptr(), ln.data_ptr(), 0, lags.data_ptr(), None, None, None, _stream(dev)),
                  "ofp_find_lags")
        cell, status = i32(B), i32(B)
        xy = torch.empty((B, 2), dtype=torch.float64, device=dev)
        rphi = torch.empty((B, 2), dtype=torch.float64, device=dev)
        res = torch.empty((B, self.side, self.side), dtype=torch.float32, device=dev) if want_res else None
        check(L.ofp_paired_vote(self.maps_dev.data_ptr(), self.map_ids.data_ptr(), self.starts.data_ptr(),
                                self.sorted_cells.data_ptr(), self.vmin.data_ptr(), self.n_buckets, S, self.side,
                                first_out.data_ptr(), lags.data_ptr(), st_in.data_ptr(), B, float(tol),
                                float(self.radius), cell.data_ptr(), xy.data_ptr(), rphi.data_ptr(), status.data_ptr(),
                                _ptr(res), _stream(dev)), "ofp_paired_vote")
        return rphi, cell, status, lags.reshape(B, 2), res

    def locate_cc(self, x, onset_idx: int, i: int, tol: int = 2, left: int = 0, right: int = 256):
        """multilateration.py:836-875: the vote over the neighbour maps of sensor i with the lags find_lag gives for
        x[onset_idx - left : onset_idx + right] ([N, C], as float32); sets ``res`` and returns
        cartesian_to_polar of the winning cell.  Refuses onset_idx - left < 0 (the reference's slice would wrap) and
        an empty window with ValueError.  Only the window travels to the device."""
        xs = x.detach() if torch.is_tensor(x) else np.asarray(x)
        if xs.ndim != 2:
            raise ValueError(f"locate_cc: x must be [N, C], got shape {tuple(xs.shape)}")
        N = xs.shape[0]
        S = len(self.sensor_locs)
        if not 0 <= int(i) < S:
            raise ValueError(f"locate_cc: sensor {i} outside 0..{S - 1}")
        if not (0 <= int(left) and int(right) >= 1 and int(left) + int(right) <= FIND_LAG_MAX_LEN):
            raise ValueError(f"locate_cc: left {left}, right {right}: need left >= 0, right >= 1 and a window of at "
                             f"most {FIND_LAG_MAX_LEN} samples")
        if int(onset_idx) - int(left) < 0:
            raise ValueError(f"locate_cc: onset_idx - left = {int(onset_idx) - int(left)} < 0")
        if min(int(onset_idx) + int(right), N) - (int(onset_idx) - int(left)) < 1:
            raise ValueError("locate_cc: empty window")  # np.correlate raises on it
        w = xs[int(onset_idx) - int(left):min(int(onset_idx) + int(right), N)]  # the window, as the reference slices
        w = w.to(torch.float32) if torch.is_tensor(w) else torch.from_numpy(np.ascontiguousarray(w, np.float32))
        xd = w.to(self.device).contiguous().unsqueeze(0)
        hits = (torch.tensor([int(left)], dtype=torch.int64, device=self.device),
                torch.tensor([int(i)], dtype=torch.int32, device=self.device), None)
        _, cell, status, _, res = self._vote(xd, hits, None, tol, left, right, want_res=True)
        st = int(status.cpu()[0])
        if st != PAIRED_OK:
            raise ValueError(f"locate_cc: window refused (status {st})")
        self.res[:] = res.cpu().numpy()[0]
        row, col = divmod(int(cell.cpu()[0]), self.side)
        xc = col - (self.side - 1) / 2
        yc = (self.side - 1) / 2 - row
        return cartesian_to_polar(xc, yc, self.radius)

    def locate_cc_device(self, x, onset_idx, first, tol: int = 2, left: int = 0, right: int = 256, clip=None):
        """``locate_cc`` for B hits at once, without host synchronisation.  x float32 CUDA [N, C] or
        [n_clips, N, C] (channel k is sensor k), onset_idx int64 CUDA [B], first int32 [B], clip int32 [B] or None
        (clip 0).  Returns rphi float64 [B, 2] (cartesian_to_polar of the cell), cell int32 [B] (flat index into
        the side x side grid; 0 when no cell matches, as np.argmax returns it) and status int32 [B]: PAIRED_OK, or
        PAIRED_NEG_WINDOW (-5, onset - left < 0), PAIRED_EMPTY_WINDOW (-6), PAIRED_BAD_HIT (-7)."""
        x = _clips(x, "locate_cc_device")
        B = onset_idx.shape[0] if torch.is_tensor(onset_idx) else -1
        for name, t, dt in (("onset_idx", onset_idx, torch.int64), ("first", first, torch.int32),
                            ("clip", clip, torch.int32)):
            if t is None and name == "clip":
                continue
            if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dt and t.dim() == 1 and t.shape[0] == B):
                raise ValueError(f"locate_cc_device: {name} must be a {dt} CUDA tensor [B]")
        hits = (onset_idx.contiguous(), first.contiguous(), clip.contiguous() if clip is not None else None)
        rphi, cell, status, _, _ = self._vote(x, hits, None, tol, left, right)
        return rphi, cell, status


    def check_stage(self, what, n_signals, tol, left, right, max_distance, min_channels):
        """The argument errors of the stream stage ("The voting locator in the hop") that need no GPU:
        host attributes only."""
        S = len(self.sensor_locs)
        if S != n_signals:
            raise ValueError(f"{what}: the locator has {S} sensors, the stream has {n_signals} signals")
        if S > _lib.REG_MAX_SIGNALS:
            raise ValueError(f"{what}: {S} sensors; the stage's grouping state holds {_lib.REG_MAX_SIGNALS}")
        if float(tol) < 0:
            raise ValueError(f"{what}: tol {tol} < 0")
        if int(left) < 0:
            raise ValueError(f"{what}: left {left} is negative")
        if int(right) < 1:
            raise ValueError(f"{what}: right {right} < 1")
        if int(left) + int(right) > _lib.PAIR_MAX_WINDOW:
            raise ValueError(f"{what}: a window of left + right = {int(left) + int(right)} samples; the stage's window "
                             f"cap is {_lib.PAIR_MAX_WINDOW}")
        lds = _lib.paired_lds_bytes(int(left) + int(right), self.side)
        if lds > _lib.PAIR_LDS_ENVELOPE:
            raise ValueError(f"{what}: the stage needs {lds} bytes of LDS (the vote bitmap of the {self.side} x {self.side} "
                             f"grid and a {int(left) + int(right)}-sample window), outside its envelope of "
                             f"{_lib.PAIR_LDS_ENVELOPE}; there is no global-memory fallback")
        if max_distance < 0:
            raise ValueError(f"{what}: max_distance {max_distance} is negative")
        if not 1 <= min_channels <= n_signals:
            raise ValueError(f"{what}: min_channels {min_channels} outside 1..{n_signals}")

    def paired_struct(self, tol=2, left=0, right=256, max_distance=1000, min_channels=3):
        """The ``ofp_hop_paired`` of this locator's index and the stage's parameters.  It points into this object's
        device tables, which must outlive whatever runs with it (a session keeps a reference to the locator)."""
        p = _lib.HopPaired()
        p.d_starts, p.d_sorted, p.d_vmin = self.starts.data_ptr(), self.sorted_cells.data_ptr(), self.vmin.data_ptr()
        p.n_buckets, p.S, p.side = self.n_buckets, len(self.sensor_locs), self.side
        p.radius, p.tol = float(self.radius), float(tol)
        p.left, p.right, p.max_distance, p.min_channels = int(left), int(right), int(max_distance), int(min_channels)
        return p

    def locate_cc_stream_device(self, audio, channels, onsets, block_size, tol=2, left=0, right=256, max_distance=1000,
                                min_channels=3):
        """What a ``HopSession(locator=self)`` would have answered on a finished recording, in ONE launch
        (``ofp_locate_cc_stream``): the stage's grouping state machine, lag search and vote over ``audio`` [N, C]
        float32 (numpy or a CUDA tensor, channel k is sensor k) and the onset list (``channels`` / ``onsets`` [K],
        absolute samples; fed sorted by sample, stable), hop by hop (N // block_size hops).  Returns a dict of per-hop
        arrays: ``hit`` bool [H], ``status`` int32 [H] (PAIRED_OK or PAIRED_NEG_WINDOW), ``onset`` int64 [H], ``first``
        int32 [H], ``group`` int64 [H, C], ``lags`` int32 [H, 2], ``cell`` int32 [H], ``rphi`` float64 [H, 2] (NaN
        where there is no hit or a status) and ``pending`` int32 [H], the FIFO's length before the hop's evaluation.
        The ring and queue conditions of a session do not apply; a queue overflow or a refused onset raises
        OnsetFPError."""
        from . import realtime
        what = "locate_cc_stream_device"
        ad = audio if torch.is_tensor(audio) else torch.from_numpy(np.ascontiguousarray(audio, dtype=np.float32))
        if ad.dim() != 2:
            raise ValueError(f"{what}: audio must be [N, C], got {tuple(ad.shape)}")
        C = int(ad.shape[1])
        self.check_stage(what, C, tol, left, right, max_distance, min_channels)
        onsets = np.asarray(onsets, dtype=np.int64).reshape(-1)
        channels = np.asarray(channels, dtype=np.int32).reshape(-1)
        if len(onsets) != len(channels):
            raise ValueError(f"{what}: {len(channels)} channels for {len(onsets)} onsets")
        order = np.argsort(onsets, kind="stable")
        onsets, channels = onsets[order], channels[order]
        dev = self.device
        ad = ad.to(dev, torch.float32).contiguous()
        H = int(ad.shape[0]) // block_size
        with torch.cuda.device(dev):
            p = self.paired_struct(tol, left, right, max_distance, min_channels)
            ch_d, on_d = torch.from_numpy(channels).to(dev), torch.from_numpy(onsets).to(dev)
            z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
            hit, status, first, cell, pending = (z(H, torch.int32) for _ in range(5))
            onset, rows, lags = z(H, torch.int64), z((H, C), torch.int64), z((H, 2), torch.int32)
            xy = torch.full((H, 2), float("nan"), dtype=torch.float64, device=dev)
            rphi = torch.full((H, 2), float("nan"), dtype=torch.float64, device=dev)
            flags = z(1, torch.int32)
            check(_lib.lib().ofp_locate_cc_stream(ctypes.byref(p), ad.data_ptr(), ad.shape[0], block_size,
                                                  ch_d.data_ptr(), on_d.data_ptr(), len(onsets), hit.data_ptr(),
                                                  status.data_ptr(), onset.data_ptr(), first.data_ptr(),
                                                  rows.data_ptr(), lags.data_ptr(), cell.data_ptr(), xy.data_ptr(),
                                                  rphi.data_ptr(), pending.data_ptr(), flags.data_ptr(), _stream(dev)),
                  "ofp_locate_cc_stream")
        realtime.check_regress_flags(int(flags.item()), what)
        return dict(hit=hit.cpu().numpy().astype(bool), status=status.cpu().numpy(), onset=onset.cpu().numpy(),
                    first=first.cpu().numpy(), group=rows.cpu().numpy(), lags=lags.cpu().numpy(),
                    cell=cell.cpu().numpy(), rphi=rphi.cpu().numpy(), pending=pending.cpu().numpy())


def _clips(x, what):
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() in (2, 3)):
        raise ValueError(f"{what}: x must be a float32 CUDA tensor [N, C] or [n_clips, N, C]")
    return (x if x.dim() == 3 else x.unsqueeze(0)).contiguous()


def locate_cc_groups_device(x, groups, n_groups, m: MultilateratePaired, tol: int = 2, left: int = 0,
                            right: int = 256):
    """``MultilateratePaired.locate_cc`` for every row of `detection.group_onsets_device`, without host
    synchronisation.  x float32 CUDA [n_clips, N, C]; groups int64 [n_clips, cap_groups, C] (channel k is sensor k,
    a negative onset is an absent channel), n_groups int64 [n_clips] or None (every row).  Per row, the first sensor
    is the earliest channel (ties by channel) and onset_idx its onset.  Returns rphi float64
    [n_clips, cap_groups, 2], cell int32 and status int32 [n_clips, cap_groups] as locate_cc_device, plus
    PAIRED_UNUSED (-1, row beyond the clip's groups) and PAIRED_NO_CHANNEL (-2)."""
    x = _clips(x, "locate_cc_groups_device")
    if not (torch.is_tensor(groups) and groups.is_cuda and groups.dtype == torch.int64 and groups.dim() == 3):
        raise ValueError("locate_cc_groups_device: groups must be an int64 CUDA tensor [n_clips, cap_groups, C]")
    n_clips, cap, C = groups.shape
    if (n_clips, C) != (x.shape[0], x.shape[2]):
        raise ValueError(f"locate_cc_groups_device: groups {tuple(groups.shape)} do not fit x {tuple(x.shape)}")
    if n_groups is not None and not (torch.is_tensor(n_groups) and n_groups.is_cuda and n_groups.dtype == torch.int64
                                     and n_groups.shape == (n_clips,)):
        raise ValueError("locate_cc_groups_device: n_groups must be an int64 CUDA tensor [n_clips]")
    if cap == 0:
        e = torch.empty((n_clips, 0), dtype=torch.int32, device=x.device)
        return torch.empty((n_clips, 0, 2), dtype=torch.float64, device=x.device), e, e.clone()
    rphi, cell, status, _, _ = m._vote(x, None, (groups.contiguous(), n_groups.contiguous() if n_groups is not None
                                                 else None), tol, left, right)
    return rphi.reshape(n_clips, cap, 2), cell.reshape(n_clips, cap), status.reshape(n_clips, cap)


# ---- lag_intensity_map --------------------------------------------------------------------------------------

def sound_intensity_at_source(strike_location, strike_force=STRIKE_FORCE, diameter=DIAMETER) -> float:
    """multilateration.py:1004-1008 (a placeholder there): the strike force."""
    return strike_force


def vec_sub(a, b):
    """multilateration.py:1011-1015: rows (a.x - b.x, a.y - b.y, a.z - b.z) for the points of b (x and y arrays,
    scalar z) -> [n, 3] float64."""
    dx = a[0] - b[0].reshape(-1)
    dy = a[1] - b[1].reshape(-1)
    dz = np.full_like(dx, a[2] - b[2], dtype=float)
    return np.vstack((dx, dy, dz)).T


def attenuate_intensity(source_loc, mic_loc, reflectivity, intensity_at_source):
    """multilateration.py:1018-1043: intensity at mic_loc of sources on the drumhead, scaled by
    1 + reflectivity * (1 - |cos theta|) over the distance (theta: angle to the surface normal), and theta in
    degrees."""
    v = vec_sub(mic_loc, source_loc)
    dist = np.linalg.norm(v, axis=-1)
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    theta = np.arccos(np.dot(v, np.array([0.0, 0.0, 1.0])))
    return intensity_at_source * (1 + reflectivity * (1 - np.abs(np.cos(theta)))) / dist, np.degrees(theta)


def lag_intensity_map(mic_a, mic_b, reflectivity: float = 0.5, d: int = DIAMETER, sr: int = 96000,
                      scale: float = 1, medium: str = MEDIUM, device=0):
    """multilateration.py:1046-1101: the lag map (samples, lag_map_3d without mask) and the two signal-strength
    maps 10 log10(attenuate_intensity) in dB, all float32 [side, side]; the lags by ``ofp_lag_maps``, the
    strengths by ``ofp_intensity_maps`` (fp64 rounded once to float32)."""
    mics = np.array([list(mic_a), list(mic_b)], dtype=np.float64)
    if mics.shape != (2, 3):
        raise ValueError(f"lag_intensity_map: microphones must be (x, y, z), got shape {mics.shape[1:]}")
    r = int(np.round(d, 1) * scale) // 2
    dev = _dev(device)
    _lib.require_gpu(dev.index or 0)
    maps, _, _ = lag_maps_device(mics[::-1], r, speed_of_sound(100 * scale, medium=medium), sr, np.inf, device=dev)
    side = 2 * r + 1
    out = torch.empty((2, side, side), dtype=torch.float32, device=dev)
    m = torch.from_numpy(np.ascontiguousarray(mics)).to(dev)
    check(_lib.lib().ofp_intensity_maps(m.data_ptr(), r, float(reflectivity), out.data_ptr(), _stream(dev)),
          "ofp_intensity_maps")
    out = out.cpu().numpy()
    return maps[0, 1].cpu().numpy(), out[0], out[1]
