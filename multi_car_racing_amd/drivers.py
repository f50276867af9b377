"""Scripted drivers (include/mcr.h: mcr_set_drivers; csrc/k_driver.h holds the controller's definition): the keyword arguments of
VecMultiCarRacing(scripted_agents=..., driver_params=...) turned into the parameter rows and the car mask of the C ABI.  No torch, no GPU:
everything here is validated on the host before a handle exists."""
import ctypes

import numpy as np

from . import _lib
from ._lib import DRIVER_DEFAULTS, DRIVER_PARAM_NAMES, DRV_PARAMS  # noqa: F401


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
