"""MI355X: the main raster (csrc/k_view.h, with the record it draws from, csrc/k_carview.h) on the synthetic scenes of tests/view_cases.py,
through a launch of its own (mcr_obs_now), against the oracle's render of the same state — exact outside the oracle's ambiguous pixels, at
most 40 edge pixels per view.  tests/test_view_cases.py holds the scenes to what they are meant to be without a device: which branch of the
candidate layout each set reaches, the ambiguity cap, the oracle's setters.

What the rollouts' frames do not reach and this file does: every block of a full road_poly in one view at t = 0 (eight rounds of
candidates, up to 400 grass squares and the playfield quad), eight cars and twelve blocks of kerbed road in one zoomed-in view (the
contiguous layout, several rounds), cars stacked, cars poking into the frame from outside on each side, cars either side of the raster's
reach, a car under the HUD bar, ego colours with eight cars; the playfield's corners and edges zoomed in, views wholly outside it; every
gauge negative, taller than the bar, out of the frame; labels up to ten digits; the flag; touched tiles in patterns; the zoom in between.

The same state goes to the device (set_bodies / set_wheels / set_env_state / refresh_flags) and to each env's oracle (set_body /
set_render_state / set_time / set_reward / set_touched / the flag read back): nothing reaches a solver on either side."""
import ctypes

import numpy as np
import pytest

from tests import obs_cases as C
from tests import view_cases as V
from tests.util import assert_frame, assert_pixels, assert_state, luma_np, make_env, oracles, random_actions

pytestmark = pytest.mark.gpu

MCR_OK, MCR_ERR_ARG, MCR_ERR_STATE = 0, -1, -3
GUARD = 4096                   # sentinel bytes in front of and behind the frames
SENTINEL = 0xA5
vp = ctypes.c_void_p


@pytest.fixture(scope="module")
def trks(lib):
    return V.tracks(lib)


class ViewRig(C.Rig):
    """reset once, stepped ONCE (just_reset is clear), never stepped again; one oracle per env on the device's own blob"""

    def __init__(self, lib, O, trks, N, **kw):
        import torch
        assert torch.cuda.is_available(), "these tests need the MI355X"
        super().__init__(lib, trks, N, "pixels", steps=1, use_ego_color=N in V.EGO_COLOR_NS, **kw)
        self.orcs, self.eps, self.vbase = V.make_oracles(lib, O, trks, N)
        self.status0 = self.env.status_words().tolist()
        self.flags0 = self.env.get_env_state()["tile_flags"]
        self.gray = kw.get("obs_format") == "gray"

    def close(self):
        for o in self.orcs:
            o.close()
        super().close()

    def draw(self, case):
        """the case into the device, mcr_obs_now into a guarded buffer; (frames [B, N, 96, 96, C], the flags the device drew)"""
        torch, env = self.torch, self.env
        env.set_bodies(case["bodies"]); env.set_wheels(case["wheels"])
        env.set_env_state(case["reward"], case["t"], V.tile_flags(self.flags0, case["touched"]))
        env.refresh_flags()
        n = self.B * self.N * 96 * 96 * (1 if self.gray else 3)
        whole = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device=env.device)
        self.held = whole
        st = torch.cuda.current_stream(env.device)
        assert env.L.mcr_obs_now(env.h, vp(whole[GUARD:].data_ptr()), vp(st.cuda_stream)) == MCR_OK, env.L.mcr_last_error()
        st.synchronize()
        h = whole.cpu().numpy()
        assert (h[:GUARD] == SENTINEL).all() and (h[-GUARD:] == SENTINEL).all(), "mcr_obs_now wrote outside its frames"
        es = env.get_env_state()
        assert np.array_equal(es["reward"], case["reward"]) and np.array_equal(es["t"], case["t"])
        return h[GUARD:-GUARD].reshape(self.B, self.N, 96, 96, -1), es["driving_backward"]

    def compare(self, set_name, transform=None):
        flags = set()
        for rnd in range(V.rounds(set_name, self.N)):
            case = V.build(self.L, self.tracks, self.N, self.vbase, set_name, rnd)
            got, bw = self.draw(case)
            flags |= set(bw.ravel().tolist())
            for e, o in enumerate(self.orcs):
                V.apply_to_oracle(o, case, e, backward=bw[e])
                want, amb = o.render_with_mask()
                want = want if transform is None else transform(want)[..., None]
                print(f"N {self.N} set {set_name} round {rnd} env {e} ({self.tracks[e][0]}): {int((got[e] != want).any(-1).sum())} pixels differ, "
                      f"{int(((got[e] != want).any(-1) & (amb == 0)).sum())} of them unambiguous; ambiguous per view {amb.reshape(self.N, -1).sum(1).tolist()}")
                assert_frame(got[e], want, amb, f"N {self.N} set {set_name} round {rnd} env {e} ({self.tracks[e][0]}, cars {case['tags'][e]})", V.BUDGET)
        assert self.env.status_words().tolist() == self.status0, "a status word was raised"
        return flags


@pytest.fixture(scope="module", params=V.NS, ids=lambda n: f"N{n}")
def rig(request, lib, oracle, trks):
    r = ViewRig(lib, oracle, trks, request.param)
    yield r
    r.close()


@pytest.fixture(scope="module", params=(2, 8), ids=lambda n: f"N{n}")
def gray_rig(request, lib, oracle, trks):
    r = ViewRig(lib, oracle, trks, request.param, obs_format="gray", frame_stack=1)
    yield r
    r.close()


def test_the_rig_is_live_and_past_its_first_step(rig):
    rec = np.zeros((rig.B, 12), np.int32)
    assert rig.L.mcr_debug_read_env_records(rig.env.h, rec.ctypes.data_as(vp), rec.nbytes) >= 0
    assert (rec[:, 6] == 1).all() and (rec[:, 8] == 0).all(), "every env active, none just reset"
    assert rig.status0[:2] == [0, 0]


@pytest.mark.parametrize("set_name", V.SETS)
def test_frames_equal_the_oracle(rig, set_name):
    flags = rig.compare(set_name)
    if set_name == "hud":
        assert flags == {0, 1}, "the backwards flag is drawn in some views and not in others"


@pytest.mark.parametrize("set_name", ("generic", "hud"))
def test_gray_frames_equal_the_luma_of_the_oracle(gray_rig, set_name):
    gray_rig.compare(set_name, transform=luma_np)


@pytest.mark.parametrize("bit,set_name", [(4, "crowd"), (2, "tiles")], ids=["without-cars", "without-road"])
def test_the_comparison_can_fail(rig, bit, set_name):
    """mcr_debug_set 4: the raster skips the cars; 2: the road_poly entries — the comparison with the oracle raises"""
    try:
        assert rig.L.mcr_debug_set(rig.env.h, bit) == MCR_OK
        with pytest.raises(AssertionError, match="unambiguous pixels differ"):
            rig.compare(set_name)
    finally:
        assert rig.L.mcr_debug_set(rig.env.h, 0) == MCR_OK
    rig.compare(set_name)


@pytest.mark.parametrize("N", (2, 4))
def test_obs_now_disturbs_nothing(lib, oracle, N):
    """a rollout with contacts on the default streams, refresh_obs() between its steps: the frame is the oracle's render of the state as it
    stands (the current reward on the label, the current flag), and the rollout goes on bit for bit in state and reward, exact in pixels"""
    import torch
    from multi_car_racing_amd.vec_env import VecMultiCarRacing
    B, seed, steps = 4, 11, 40
    env = VecMultiCarRacing(B, N, seed=seed, car_contacts=True, async_refill=False, use_random_direction=False, auto_reset=False, max_episode_steps=0, obs=True)
    orcs = oracles(oracle, B, N, seed)
    try:
        obs = env.reset().cpu().numpy()
        assert_pixels(obs, orcs)
        rng = np.random.RandomState(3)
        own = torch.zeros_like(env.obs)
        for k in range(steps):
            a = random_actions(rng, B, N, brake_scale=0.2)
            obs, rew, done, _ = env.step(torch.from_numpy(a).to(env.device))
            obs = obs.cpu().numpy(); rew = rew.cpu().numpy()
            for e, o in enumerate(orcs):
                _, r, d, _ = o.step(a[e], render=True)
                assert np.array_equal(r, rew[e]) and not d, f"step {k} env {e}"
            assert_pixels(obs, orcs)
            if k % 3 != 2:
                now = env.refresh_obs(own if k % 2 else None)
                assert (now is own) == bool(k % 2)
                torch.cuda.synchronize()
                now = now.cpu().numpy()
                for e, o in enumerate(orcs):
                    want, amb = o.render_with_mask()
                    assert_frame(now[e], want, amb, f"refresh_obs behind step {k}, env {e}", V.BUDGET)
        assert_state(env, list(enumerate(orcs)), f"after {steps} steps")
        assert env.status_words()[:2].tolist() == [0, 0]
    finally:
        env.close()
        for o in orcs:
            o.close()


def test_error_returns(lib):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    L = lib.load()
    buf = torch.zeros((2, 2, 96, 96, 3), dtype=torch.uint8, device="cuda")
    assert L.mcr_obs_now(None, vp(buf.data_ptr()), None) == MCR_ERR_ARG
    env = make_env(2, 2, 5, obs=True)
    try:
        st = torch.cuda.current_stream(env.device)
        assert L.mcr_obs_now(env.h, None, vp(st.cuda_stream)) == MCR_ERR_ARG
        assert L.mcr_obs_now(env.h, vp(buf.data_ptr()), vp(st.cuda_stream)) == MCR_ERR_STATE and b"before reset" in L.mcr_last_error()
        env.reset()
        assert L.mcr_obs_now(env.h, vp(buf.data_ptr()), vp(st.cuda_stream)) == MCR_OK
        st.synchronize()
        assert np.array_equal(buf.cpu().numpy(), env.obs.cpu().numpy()), "behind reset() alone the frame is the reset's"
        side = torch.cuda.Stream(env.device)
        scratch = torch.zeros(16, device=env.device)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            scratch.add_(1.0)
            rc = L.mcr_obs_now(env.h, vp(buf.data_ptr()), vp(torch.cuda.current_stream(env.device).cuda_stream))
            msg = L.mcr_last_error()
        assert rc == MCR_ERR_STATE and b"capture" in msg
        assert L.mcr_set_wheels(env.h, None) == MCR_ERR_ARG and L.mcr_set_wheels(None, None) == MCR_ERR_ARG and L.mcr_set_env_state(None, None, None, None) == MCR_ERR_ARG
        before = env.get_env_state(), env.get_state()
        assert L.mcr_set_env_state(env.h, None, None, None) == MCR_OK
        env.set_wheels(before[1]["wheels"]); env.set_env_state(before[0]["reward"], before[0]["t"], before[0]["tile_flags"])
        after = env.get_env_state(), env.get_state()
        for b, a in zip(before, after):
            for k in b:
                assert np.array_equal(b[k], a[k]), k
        w = before[1]["wheels"].copy(); w[..., :3] = 7.0; w[..., 3] += 1.5; w[..., 4] -= 2.5
        env.set_wheels(w)
        got = env.get_state()["wheels"]
        assert np.array_equal(got[..., 3:], w[..., 3:]) and np.array_equal(got[..., :3], before[1]["wheels"][..., :3]), "phase and omega written, the controls ignored"
    finally:
        env.close()
    for kw, what in ((dict(obs=False), b"obs_enabled"), (dict(obs=True, obs_format="gray", frame_stack=2), b"stacked")):
        env = make_env(2, 2, 5, **kw)
        try:
            env.reset()
            st = torch.cuda.current_stream(env.device)
            assert L.mcr_obs_now(env.h, vp(buf.data_ptr()), vp(st.cuda_stream)) == MCR_ERR_STATE and what in L.mcr_last_error()
            with pytest.raises(lib.McrError):
                env.refresh_obs()
        finally:
            env.close()
