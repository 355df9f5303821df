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

Batched, device-resident addition: ``locate_groups_device`` locates every onset group ``group_onsets_device``
found, in one pass without host synchronisation.

Out of scope: the 2-D ``Multilaterate`` and ``MultilateratePaired`` classes, ``lag_intensity_map``,
``find_lag_multi`` and the other helpers of the reference file.  There is no CPU path: every GPU function raises
without the library or a gfx950 GPU.
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


# ---- Multilaterate3D ----------------------------------------------------------------------------------------

class Multilaterate3D:
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
        sensors = _sensor_array(self.sensor_locs)
        self.device = _dev(device)
        _lib.require_gpu(self.device.index or 0)
        S = len(sensors)
        r, mask_r2 = _grid_3d(drum_diameter, 1, 2)
        self.grid_radius = r
        self.maps_dev, self.min_dev, self.max_dev = lag_maps_device(
            sensors, r, self.c, sr, mask_r2, floor=-self.samples_per_cm * 1, device=self.device)
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
        """multilateration.py:413-426: (col, row) of the first map cell consistent with both lags of the group
        within `tolerance` cm, (0, 0) when there is none."""
        sensors, onsets = group[0], group[1]
        s = torch.tensor([[int(v) for v in sensors[:3]]], dtype=torch.int32, device=self.device)
        o = torch.tensor([[int(v) for v in onsets[:3]]], dtype=torch.int64, device=self.device)
        idx = legal_cells_device(self.maps_dev, s, o, tolerance * self.samples_per_cm).cpu().numpy()[0]
        return int(idx[0]), int(idx[1])

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


# ---- batched offline locator --------------------------------------------------------------------------------

def locate_groups_device(groups, n_groups, m: Multilaterate3D, xtol=XTOL, maxfev=MAXFEV, return_guess=False):
    """Locate every onset group of a batch on the device, without host synchronisation.

    groups int64 CUDA [n_clips, cap_groups, C] and n_groups int64 [n_clips] (or None: every row), as
    `detection.group_onsets_device` returns them (optionally after `detection.fix_onsets_device`); channel k is
    sensor k of `m` (C <= number of sensors).  Per row, the reference's own steps in the order
    ``Multilaterate3D.locate`` applies them: the three earliest channels present, ordered by onset (ties by channel
    index), are origin, a and b; ``is_legal(origin, a)`` and ``is_legal(origin, b)``; ``is_legal_3d``;
    ``trilaterate`` from the guess (col, row) - radius, with its reordering (or ``m.model``).

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
    if m.model is not None:
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
    check(L.ofp_locate_groups(groups.data_ptr(), n_clips, cap, C, _ptr(n_groups), m.sensors_dev.data_ptr(),
                              m.sensors_dev.shape[0], m.maps_dev.data_ptr(), m.min_dev.data_ptr(), m.max_dev.data_ptr(),
                              m.grid_radius, float(m.samples_per_cm), float(m.sr), float(m.c), float(m.radius),
                              float(xtol), int(maxfev), mlp.handle if mlp is not None else None, xy.data_ptr(),
                              status.data_ptr(), _ptr(guess), ws.data_ptr(), ws.numel(), _stream(dev)),
          "ofp_locate_groups")
    return (xy, status, guess) if return_guess else (xy, status)
