"""Scripted drivers (include/mcr.h: mcr_set_drivers; csrc/k_driver.h holds the controller's definition): the keyword arguments of
VecMultiCarRacing(scripted_agents=..., driver_params=...) turned into the parameter rows and the car mask of the C ABI.  No torch, no GPU:
everything here is validated on the host before a handle exists."""
import ctypes

import numpy as np

from . import _lib
from ._lib import DRIVER_DEFAULTS, DRIVER_PARAM_NAMES, DRV_PARAMS, RACECRAFT_DEFAULTS, RACECRAFT_PARAM_NAMES, RC_PARAMS  # noqa: F401


def default_params(num_agents):
    """[N, 10] float32: the default row for every car"""
    return np.tile(np.asarray([DRIVER_DEFAULTS[k] for k in DRIVER_PARAM_NAMES], np.float32), (int(num_agents), 1))


def driver_mask(num_agents, scripted_agents):
    """a sequence of car indices (None or (): none) -> bit mask; ValueError for an index outside 0 .. N-1, a duplicate, or a non-integer"""
    if scripted_agents is None:
        return 0
    if isinstance(scripted_agents, (str, bytes)) or not hasattr(scripted_agents, "__iter__"):
        raise ValueError(f"scripted_agents must be a sequence of car indices, got {scripted_agents!r}")
    mask = 0
    for a in scripted_agents:
        if isinstance(a, bool) or not isinstance(a, (int, np.integer)):
            raise ValueError(f"scripted_agents must hold integers, got {a!r}")
        if not 0 <= int(a) < int(num_agents):
            raise ValueError(f"scripted_agents: car {int(a)} is outside 0..{int(num_agents) - 1}")
        if mask >> int(a) & 1:
            raise ValueError(f"scripted_agents lists car {int(a)} twice")
        mask |= 1 << int(a)
    return mask


def driver_params_array(num_agents, driver_params=None):
    """None (the defaults for every car), a dict of overrides {name: scalar or per-car sequence}, or a float array [N, 10] -> the validated
    [N, 10] float32 rows (a copy).  ValueError for an unknown name, a wrong shape, or a value mcr_set_drivers would refuse."""
    N = int(num_agents)
    rows = default_params(N)
    if isinstance(driver_params, dict):
        for name, v in driver_params.items():
            if name not in DRIVER_PARAM_NAMES:
                raise ValueError(f"driver_params: unknown parameter {name!r} (one of {', '.join(DRIVER_PARAM_NAMES)})")
            try:
                col = np.asarray(v, np.float64)
            except (TypeError, ValueError):
                raise ValueError(f"driver_params[{name!r}] must be a number or a sequence of {N} numbers, got {v!r}") from None
            if col.ndim > 1 or (col.ndim == 1 and col.shape[0] != N):
                raise ValueError(f"driver_params[{name!r}] must be a number or a sequence of {N} numbers, got shape {col.shape}")
            rows[:, DRIVER_PARAM_NAMES.index(name)] = col.astype(np.float32)
    elif driver_params is not None:
        try:
            arr = np.asarray(driver_params, np.float64)
        except (TypeError, ValueError):
            raise ValueError("driver_params must be None, a dict of overrides or a float array [num_agents, 10]") from None
        if arr.shape != (N, DRV_PARAMS):
            raise ValueError(f"driver_params must have shape ({N}, {DRV_PARAMS}), got {arr.shape}")
        rows = arr.astype(np.float32)
    rows = np.ascontiguousarray(rows, np.float32)
    L = _lib.load()
    if L.mcr_check_drivers(N, _lib.ptr(rows), ctypes.c_uint32(0)) != 0:
        raise ValueError(L.mcr_last_error().decode())
    return rows


def default_racecraft_params(num_agents):
    """[N, 8] float32: the default racecraft row for every car"""
    return np.tile(np.asarray([RACECRAFT_DEFAULTS[k] for k in RACECRAFT_PARAM_NAMES], np.float32), (int(num_agents), 1))


def racecraft_params_array(num_agents, racecraft=True, scripted_mask=0):
    """VecMultiCarRacing's `racecraft` keyword -> (rows [N, 8] float32, car mask), or (None, 0) for None / False.  True: the defaults; a dict
    {name: scalar or per-car sequence} of overrides, optionally with "agents": the cars that race; a float array [N, 8].  Without "agents"
    the cars of `scripted_mask` race, or every car when that is 0 (expert labels only).  ValueError for an unknown name, a wrong shape, a
    car outside 0 .. N-1 or a value mcr_set_racecraft would refuse."""
    N = int(num_agents)
    if racecraft is None or racecraft is False:
        return None, 0
    rows = default_racecraft_params(N)
    mask = int(scripted_mask) if scripted_mask else (1 << N) - 1
    if racecraft is True:
        pass
    elif isinstance(racecraft, dict):
        for name, v in racecraft.items():
            if name == "agents":
                try:
                    mask = driver_mask(N, v)
                except ValueError as e:
                    raise ValueError(str(e).replace("scripted_agents", "racecraft['agents']")) from None
                continue
            if name not in RACECRAFT_PARAM_NAMES:
                raise ValueError(f"racecraft: unknown parameter {name!r} (one of {', '.join(RACECRAFT_PARAM_NAMES)}, agents)")
            try:
                col = np.asarray(v, np.float64)
            except (TypeError, ValueError):
                raise ValueError(f"racecraft[{name!r}] must be a number or a sequence of {N} numbers, got {v!r}") from None
            if col.ndim > 1 or (col.ndim == 1 and col.shape[0] != N):
                raise ValueError(f"racecraft[{name!r}] must be a number or a sequence of {N} numbers, got shape {col.shape}")
            rows[:, RACECRAFT_PARAM_NAMES.index(name)] = col.astype(np.float32)
    else:
        try:
            arr = np.asarray(racecraft, np.float64)
        except (TypeError, ValueError):
            raise ValueError("racecraft must be None, a bool, a dict of overrides or a float array [num_agents, 8]") from None
        if arr.shape != (N, RC_PARAMS):
            raise ValueError(f"racecraft must be None, a bool, a dict of overrides or a float array of shape ({N}, {RC_PARAMS}), got {arr.shape}")
        rows = arr.astype(np.float32)
    rows = np.ascontiguousarray(rows, np.float32)
    L = _lib.load()
    if L.mcr_check_racecraft(N, _lib.ptr(rows), ctypes.c_uint32(0)) != 0:
        raise ValueError(L.mcr_last_error().decode())
    return rows, mask
