"""Data-parallel env sharding: one process per GPU, contiguous env slices, no data-path
collective.  The only communication is a tiny SUM/MAX all-reduce of rollout metrics (RCCL over xGMI when the
process group backend is "nccl"; gloo on CPU in the tests)."""
import numpy as np


def shard_range(total_envs, rank, world_size):
    """Contiguous slice [lo, hi) of the global env index space owned by `rank` (sizes differ by at most 1)."""
    base, rem = divmod(int(total_envs), int(world_size))
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def reduce_metrics(env_steps, elapsed_s, episodes=0.0, return_sum=0.0, group=None):
    """All-reduce rollout metrics: SUM of env_steps/episodes/return_sum, MAX of elapsed seconds.
    Returns dict with the job-wide values (identical on every rank).  Works without torch.distributed
    (single process) by returning the local values."""
    import torch
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return dict(env_steps=float(env_steps), elapsed_s=float(elapsed_s), episodes=float(episodes),
                    return_sum=float(return_sum), world_size=1)
    dev = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend(group) == "nccl" else torch.device("cpu")
    sums = torch.tensor([env_steps, episodes, return_sum], dtype=torch.float64, device=dev)
    mx = torch.tensor([elapsed_s], dtype=torch.float64, device=dev)
    dist.all_reduce(sums, op=dist.ReduceOp.SUM, group=group)
    dist.all_reduce(mx, op=dist.ReduceOp.MAX, group=group)
    s = sums.cpu().numpy(); m = mx.cpu().numpy()
    return dict(env_steps=float(s[0]), elapsed_s=float(m[0]), episodes=float(s[1]), return_sum=float(s[2]),
                world_size=dist.get_world_size(group))


class ShardedVecEnv:
    """This rank's slice of a job-wide batch of `total_envs` environments.  Env g (global index) behaves
    identically whatever the world size because its RNG streams are keyed by g (vec_env.py).  Every keyword of
    VecMultiCarRacing passes through (`state_obs`, `state_waypoints`, `state_stride`, `range_obs`, `range_rays`, `range_fov`, `range_angles`, `range_max`, `contact_obs`, `grid_obs`, `grid_shape`, `grid_cell`, `grid_origin`, `end_patience`, `end_offroad`, `end_offroad_mode`, `end_agents`, `end_reward`, `frame_skip`, `levels`, `level_seed`, `level_order`
    included: every rank makes the same pool, and an env's levels follow its GLOBAL index — under `level_order="weighted"` too, provided every
    rank calls `set_level_weights` with the same weights at the same steps; `level_stats`: each rank accumulates ITS slice's episodes in its own
    `level_stats` — a caller may all_reduce the tensor, after which the sums are no longer bit-identical across world sizes; `scripted_agents`, `driver_params`: the scripted
    driver is a pure function of an env's state, so a car drives the same whatever rank holds its env) and every attribute
    and method of the slice is reachable here (`state`, `state_shape`, `ranges`, `range_shape`, `range_angles`, `range_dirs`, `refresh_ranges()`, `grid`, `grid_shape`, `grid_cell`, `grid_origin`, `refresh_grid()`, `grid_planes()`, `contact_mask`, `contact_impulse`, `refresh_contacts()`, `end_counters`, `end_reason`, `refresh_end_rules()`, `frame_skip`, `refresh_state()`, `actions`, `driver_params`,
    `expert_actions()`: this rank's rows)."""

    def __init__(self, total_envs, num_agents=2, seed=0, rank=0, world_size=1, device=None, **kw):
        from .vec_env import VecMultiCarRacing
        self.rank, self.world_size = rank, world_size
        self.lo, self.hi = shard_range(total_envs, rank, world_size)
        self.env = VecMultiCarRacing(self.hi - self.lo, num_agents, device=device, seed=seed, env_offset=self.lo,
                                     world_size=world_size, **kw)

    def __getattr__(self, name):
        return getattr(self.env, name)
