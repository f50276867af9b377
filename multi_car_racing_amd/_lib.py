"""ctypes binding of include/mcr.h.  Fails loudly if the HIP library is missing — there is no CPU fallback."""
import ctypes, os
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MCR_LIB_PATH") or os.path.join(HERE, "_lib", "libmcr_hip.so")      # (MCR_LIB_PATH: another build of the same ABI, for A/B measurements)

MAX_AGENTS = 8
TILE_CAP = 512
QUAD_CAP = 768
MT_WORDS = 625
OBS_RGB, OBS_GRAY, OBS_STACK_MAX = 0, 1, 8
REPEAT_MAX = 16                 # include/mcr.h: MCR_REPEAT_MAX
RANGE_RAYS_MAX = 32             # include/mcr.h: MCR_RANGE_RAYS_MAX, rays per car of the range-finder observation
GRID_MAX = 64                   # include/mcr.h: MCR_GRID_MAX, rows and columns per car of the grid observation
GRID_ROAD, GRID_FRESH, GRID_TAKEN, GRID_CAR = 1, 2, 4, 8        # include/mcr.h: MCR_GRID_*, the bits of a grid cell
DRV_PARAMS = 10                 # include/mcr.h: MCR_DRV_PARAMS, floats per parameter row of a scripted driver
DRIVER_PARAM_NAMES = ("L1", "L2", "v_max", "K_s", "K_c", "K_g", "K_b", "offset", "gas_max", "brake_max")
DRIVER_DEFAULTS = dict(zip(DRIVER_PARAM_NAMES, (4.0, 12.0, 70.0, 8.0, 20.0, 0.2, 0.1, 0.0, 1.0, 0.8)))    # include/mcr.h: MCR_DRV_DEFAULTS
RC_PARAMS = 8                   # include/mcr.h: MCR_RC_PARAMS, floats per racecraft row of a scripted driver
RACECRAFT_PARAM_NAMES = ("look", "w_block", "w_pass", "off_max", "d_safe", "K_f", "w_off", "v_off")
RACECRAFT_DEFAULTS = dict(zip(RACECRAFT_PARAM_NAMES, (24.0, 3.5, 4.25, 4.5, 16.0, 2.0, 7.5, 15.0)))        # include/mcr.h: MCR_RC_DEFAULTS
LEVEL_ORDER = {"random": 0, "cycle": 1}      # include/mcr.h: mcr_set_episode_pool's mode ("weighted" is no mode: vec_env.py puts a sampler on a mode-0 pool)

# mcr_debug_set bits: the mirror of enum McrDebugBit (csrc/mcr_kernels.h, which says what each one does; tests/test_abi.py compares the two)
DEBUG_VIEW_CLOCKS = 1 << 5
DEBUG_POS_ITERS_2 = 1 << 6
DEBUG_VEL_ITERS_2 = 1 << 7
DEBUG_DYN_CLOCKS = 1 << 8
DEBUG_NO_CC_VELOCITY = 1 << 9
DEBUG_NO_CC_EXCHANGE = 1 << 10
DEBUG_EPOCH_ACQ_REL = 1 << 11
DEBUG_STARVED_COLLIDE = 1 << 12
DEBUG_SHORT_AWAIT = DEBUG_SHORT_EPOCH_WAIT = DEBUG_WITHHOLD_ENV0_EPOCH = DEBUG_STARVED_COLLIDE
DEBUG_NO_SIDE_POST = 1 << 13
DEBUG_OLD_SOLVE_ORDER = 1 << 14
DEBUG_COLLIDE_CLOCKS = 1 << 15
DEBUG_DYN_CLOCKS_VEL = 1 << 16
DEBUG_TRACE = 1 << 17
DEBUG_SLOW_COLLIDE = 1 << 18
DEBUG_FLAGS_IN_STEP = 1 << 19
DEBUG_DROP_PENDING_FLAGS = 1 << 20

_vp, _i, _d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double


class Config(ctypes.Structure):
    _fields_ = [("num_envs", ctypes.c_int32), ("num_agents", ctypes.c_int32), ("device", ctypes.c_int32),
                ("obs_enabled", ctypes.c_int32), ("auto_reset", ctypes.c_int32), ("backwards_flag", ctypes.c_int32),
                ("use_ego_color", ctypes.c_int32), ("car_contacts", ctypes.c_int32), ("max_episode_steps", ctypes.c_int32),
                ("num_streams", ctypes.c_int32), ("h_ratio", ctypes.c_double),
                ("skid_particles", ctypes.c_int32), ("fresh_world", ctypes.c_int32)]


# every symbol include/mcr.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "mcr_last_error": (ctypes.c_char_p, []),
    "mcr_version": (ctypes.c_char_p, []),
    "mcr_create": (_i, [ctypes.POINTER(Config), ctypes.POINTER(_vp)]),
    "mcr_destroy": (_i, [_vp]),
    "mcr_episode_bytes": (ctypes.c_size_t, []),
    "mcr_mt_seed": (None, [_vp, ctypes.c_uint32]),
    "mcr_mt_seed_by_array": (None, [_vp, _vp, _i]),
    "mcr_mt_random_sample": (_d, [_vp]),
    "mcr_mt_choice_cw": (_i, [_vp]),
    "mcr_mt_car_order": (None, [_vp, _i, _vp]),
    "mcr_episode_generate": (_i, [_vp, _i, _i, _vp, _vp, _vp]),
    "mcr_episodes_generate": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _i]),
    "mcr_episodes_generate_rows": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _i]),
    "mcr_episode_from_track": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp]),
    "mcr_episode_unpack": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mcr_stage_episodes": (_i, [_vp, _vp, _i, _vp, _vp]),
    "mcr_pool_level": (ctypes.c_int32, [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int32, _i]),
    "mcr_set_episode_pool": (_i, [_vp, _vp, _i, ctypes.c_uint64, ctypes.c_uint32, _i, _vp]),
    "mcr_level_cdf": (_i, [_vp, _i, _vp]),
    "mcr_pool_level_weighted": (ctypes.c_int32, [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, _vp, ctypes.c_int32]),
    "mcr_set_level_sampler": (_i, [_vp, _vp, _vp]),
    "mcr_level_weights": (_i, [_vp, _vp, _vp, _vp]),
    "mcr_level_stats_dim": (_i, [_i]),
    "mcr_set_level_stats": (_i, [_vp, _vp, _vp]),
    "mcr_reset": (_i, [_vp, _vp, _vp, _vp]),
    "mcr_step": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mcr_step_repeat": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "mcr_poll_consumed": (_i, [_vp, _vp, _i, _vp]),
    "mcr_refill_start": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp]),
    "mcr_refill_stop": (_i, [_vp]),
    "mcr_refill_wait": (_i, [_vp]),
    "mcr_refill_lag": (_i, [_vp]),
    "mcr_refill_hold": (_i, [_vp, _i]),
    "mcr_refill_generated": (ctypes.c_longlong, [_vp]),
    "mcr_refill_debug": (_i, [_vp, _vp]),
    "mcr_get_state": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mcr_set_bodies": (_i, [_vp, _vp]),
    "mcr_get_env_state": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mcr_flags_now": (_i, [_vp, _vp]),
    "mcr_set_wheels": (_i, [_vp, _vp]),
    "mcr_set_env_state": (_i, [_vp, _vp, _vp, _vp]),
    "mcr_obs_now": (_i, [_vp, _vp, _vp]),
    "mcr_get_positions": (_i, [_vp, _vp]),
    "mcr_mass_props": (None, [_vp]),
    "mcr_sincos_host": (None, [ctypes.c_float, _vp, _vp]),
    "mcr_sincos_device": (_i, [_vp, _vp, _vp, _vp, _i, _vp]),
    "mcr_timing_enable": (_i, [_vp, _i]),
    "mcr_debug_set": (_i, [_vp, _i]),
    "mcr_debug_read_view_scratch": (_i, [_vp, _i, _vp, _i]),
    "mcr_set_episode_stats": (_i, [_vp, _vp, _vp]),
    "mcr_set_terminal_obs": (_i, [_vp, _vp, _vp, _vp, _i]),
    "mcr_set_obs_format": (_i, [_vp, _i, _i]),
    "mcr_obs_bytes_per_view": (ctypes.c_size_t, [_vp]),
    "mcr_obs_window": (_i, [_vp]),
    "mcr_state_obs_dim": (_i, [_i, _i]),
    "mcr_set_state_obs": (_i, [_vp, _vp, _i, _i]),
    "mcr_state_obs_now": (_i, [_vp, _vp]),
    "mcr_check_range_obs": (_i, [_vp, _i, ctypes.c_float]),
    "mcr_set_range_obs": (_i, [_vp, _vp, _vp, _i, ctypes.c_float]),
    "mcr_range_obs_now": (_i, [_vp, _vp]),
    "mcr_check_grid_obs": (_i, [_i, _i, ctypes.c_float, ctypes.c_float, ctypes.c_float]),
    "mcr_set_grid_obs": (_i, [_vp, _vp, _i, _i, ctypes.c_float, ctypes.c_float, ctypes.c_float]),
    "mcr_grid_obs_now": (_i, [_vp, _vp]),
    "mcr_set_contact_obs": (_i, [_vp, _vp, _vp]),
    "mcr_contact_obs_now": (_i, [_vp, _vp]),
    "mcr_set_end_rules": (_i, [_vp, _i, _i, _i, ctypes.c_uint32, _d, _vp, _vp, _vp]),
    "mcr_check_end_rules": (_i, [_i, _i, _i, _i, ctypes.c_uint32, _d]),
    "mcr_end_rules_now": (_i, [_vp, _vp]),
    "mcr_contact_store_words": (_i, [_vp, _vp]),
    "mcr_hull_polygons": (_i, [_vp, _vp]),
    "mcr_driver_defaults": (_i, [_vp]),
    "mcr_check_drivers": (_i, [_i, _vp, ctypes.c_uint32]),
    "mcr_set_drivers": (_i, [_vp, _vp, ctypes.c_uint32, _vp]),
    "mcr_driver_actions": (_i, [_vp, _vp, ctypes.c_uint32, _vp, _vp]),
    "mcr_racecraft_defaults": (_i, [_vp]),
    "mcr_check_racecraft": (_i, [_i, _vp, ctypes.c_uint32]),
    "mcr_set_racecraft": (_i, [_vp, _vp, ctypes.c_uint32]),
    "mcr_read_rollout_stats": (_i, [_vp, _vp, _i]),
    "mcr_render": (_i, [_vp, _i, _i, _i, _vp, _vp]),
    "mcr_debug_read_contact_counts": (_i, [_vp, _vp]),
    "mcr_debug_read_contacts": (_i, [_vp, _vp]),
    "mcr_debug_contact_obs": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp]),
    "mcr_debug_read_tile_touch": (_i, [_vp, _vp]),
    "mcr_debug_read_proxy_ids": (_i, [_vp, _i, _vp, _i]),
    "mcr_debug_read_env_records": (_i, [_vp, _vp, _i]),
    "mcr_debug_read_partition": (_i, [_vp, _vp, _vp]),
    "mcr_debug_next_verdicts": (_i, [_vp, _i, _vp]),
    "mcr_debug_read_counters": (_i, [_vp, _vp]),
    "mcr_debug_read_counters8": (_i, [_vp, _vp]),
    "mcr_debug_read_verdict_mismatches": (_i, [_vp, _vp]),
    "mcr_concurrent_collide": (_i, [_vp]),
    "mcr_step_ordering": (_i, [_vp]),
    "mcr_step_ordering_for": (_i, [_vp, _vp]),
    "mcr_bind_stream": (_i, [_vp, _vp]),
    "mcr_debug_overlap": (_i, [_vp, _i, _vp, _vp, _i, _vp]),
    "mcr_debug_level_stats": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "mcr_status": (_i, [_vp, _vp, _i]),
    "mcr_world_create": (_vp, [_i]),
    "mcr_world_destroy": (None, [_vp]),
    "mcr_world_reset": (_i, [_vp, _vp]),
    "mcr_world_step": (_i, [_vp, _vp]),
    "mcr_world_proxy_ids": (_i, [_vp, _vp, _i]),
    "mcr_debug_read_dynamics_stamps": (_i, [_vp, _vp, _i]),
    "mcr_timing_read": (_i, [_vp, _vp, _vp]),
    "mcr_set_step_graph": (_i, [_vp, _i]),
    "mcr_state_blob_bytes": (ctypes.c_size_t, [_vp]),
    "mcr_get_state_blob": (_i, [_vp, _i, _vp]),
    "mcr_set_state_blob": (_i, [_vp, _i, _vp]),
    "mcr_state_blob_pitch": (ctypes.c_size_t, [_vp]),
    "mcr_state_blob_header": (_i, [_vp, _vp]),
    "mcr_save_states": (_i, [_vp, _vp, _i, _vp, _vp]),
    "mcr_load_states": (_i, [_vp, _vp, _i, _vp, _vp, _vp]),
    "mcr_copy_states": (_i, [_vp, _vp, _vp, _i, _vp]),
    "mcr_synth_actions": (_i, [_vp, _vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, _vp]),
    "mcr_synth_actions_block": (_i, [_vp, _vp, ctypes.c_uint64, ctypes.c_uint32, _i, ctypes.c_uint32, _vp]),
    "mcr_synth_actions_host": (None, [_vp, _i, _i, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32]),
}

_lib = None


class McrError(RuntimeError):
    pass


class McrWarning(UserWarning):
    """the build works, but not the way its numbers were measured (e.g. a second handle on a device orders its streams with events)"""


def load():
    """dlopen the in-tree library.  Import torch FIRST in GPU processes so both share one libamdhip64."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise McrError(f"{LIB_PATH} is missing: run `python -m multi_car_racing_amd.build` "
                       "(hipcc --offload-arch=gfx950). There is no CPU fallback for the step path.")
    try:
        # PyTorch-ROCm bundles its own libamdhip64.so.7; load it FIRST so that this library (same soname)
        # binds to the same HIP runtime instance that owns torch's device memory and streams.
        import torch  # noqa: F401
    except Exception:
        pass
    L = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(L, name)           # AttributeError here == header/library mismatch
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def effective_cpus():
    """CPUs this process may actually use: min(affinity mask, cgroup v2/v1 CPU quota)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            n = min(n, max(1, int(int(q) / int(per))))
    except Exception:
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read()); per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                n = min(n, max(1, q // per))
        except Exception:
            pass
    return max(1, n)


def check(rc, what=""):
    if rc < 0:
        raise McrError(f"{what} failed ({rc}): {load().mcr_last_error().decode()}")
    return rc


def ptr(a):
    """host numpy array -> void*"""
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(ctypes.c_void_p)


def episode_bytes():
    return int(load().mcr_episode_bytes())


def state_obs_dim(num_agents, waypoints=6):
    """features per car of the state-vector observation (include/mcr.h: mcr_state_obs_dim): 18 + 2 * waypoints + 4 * (num_agents - 1)"""
    return check(load().mcr_state_obs_dim(int(num_agents), int(waypoints)), "mcr_state_obs_dim")


def contact_store_words():
    """(records kept per env, u32 words of an env's car<->car manifold store, words per record) — include/mcr.h: mcr_contact_store_words"""
    per_env, per_rec = ctypes.c_int32(), ctypes.c_int32()
    cap = load().mcr_contact_store_words(ctypes.byref(per_env), ctypes.byref(per_rec))
    return int(cap), per_env.value, per_rec.value


def unpack_episode(blob):
    """host blob (uint8 array) -> dict(track (T,3) x,y,beta; quads (P,4,2) f32; quad_meta (P,) u32; spawn (8,3); cw)"""
    L = load()
    T, P, cw = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    L.mcr_episode_unpack(ptr(blob), ctypes.byref(T), ctypes.byref(P), ctypes.byref(cw), None, None, None, None, None)
    track = np.zeros((T.value, 3)); quads = np.zeros((P.value, 8), np.float32); meta = np.zeros(P.value, np.uint32)
    spawn = np.zeros((MAX_AGENTS, 3)); alpha = np.zeros(T.value)
    L.mcr_episode_unpack(ptr(blob), None, None, None, ptr(track), ptr(quads), ptr(meta), ptr(spawn), ptr(alpha))
    return dict(T=T.value, P=P.value, cw=bool(cw.value), track=track, alpha=alpha, quads=quads.reshape(-1, 4, 2),
                quad_meta=meta, spawn=spawn)
