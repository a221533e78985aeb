"""A world track on the GPU (include/ikflow_amd_track.h; ikflow_amd/csrc/track_kernels.hip, track_math.h, api_track.hip, the TRACK form of
k_sweep_edges and the node sink in run_path): calls a track must not change, the fine frames against the numpy fp64 restatement, the node kernel and
the edge mask against the fp64 references of tests/track_helpers.py, the path call against its parts bit for bit, an obstacle that is in the way
only between two key frames, handle behaviour and the Python wrappers.

Tolerances are the project's: world_helpers.CLEARANCE_TOL and PAIR_AMBIGUITY on a clearance and its closest pair, world_helpers.BAND (1e-4) around
a threshold, inside which a verdict is not compared; tests/test_track_math_host.py checks on the CPU, from the references alone, that this leaves at
most 2 % of a mask case's edges undecided and between 10 % and 90 % surely blocked."""
import ctypes as C

import numpy as np
import pytest
import torch

import cloud_helpers as CH
import helpers as H
import path_helpers as PH
import rank_helpers as RH
import sweep_helpers as SH
import track_helpers as TH
import world_helpers as WH
from ikflow_amd import _lib
from ikflow_amd.engine import EngineError
from test_path import OUTPUTS, _path, _popt, _rank, _rank_opt
from test_ranked import DEV, GUARD, _small_model_back  # noqa: F401  (a fixture)
from test_sweep import _admissible_edge_counts, _check_against_masked_dp
from test_world import _DTYPES, _FILL, _USED, _check_against_reference, _eng, _eng_model, _untouched
from test_world import OUTPUTS as CLEARANCE_OUTPUTS

pytestmark = pytest.mark.gpu
INF = np.float32(np.inf)


@pytest.fixture(autouse=True)
def _nothing_left_behind():
    yield
    for eng in _USED:   # (the engines are shared with the other test modules)
        eng.clear_world_track()
        eng.set_path_sweep(0)
        eng.clear_world()
        eng.clear_world_cloud()


def _track_clearance(eng, q, T, k, null=(), stream=None, expect=_lib.IKF_OK):
    """ikf_world_track_clearance through eng.lib on guarded buffers -> {name: cpu numpy window}."""
    n = q.shape[0]
    bufs = {o: torch.full((n + 2 * GUARD,), _FILL[o], dtype=_DTYPES[o], device=DEV) for o in CLEARANCE_OUTPUTS if o not in null}
    ptr = [bufs[o][GUARD:].data_ptr() if o in bufs else None for o in CLEARANCE_OUTPUTS]
    qd = q.to(DEV).contiguous()
    torch.cuda.synchronize()
    s = C.c_void_p(stream.cuda_stream) if stream is not None else C.c_void_p(0)
    code = eng.lib.ikf_world_track_clearance(eng._h, qd.data_ptr(), T, k, *ptr, s)
    assert code == expect, (code, _lib.last_error(eng.lib))
    torch.cuda.synchronize()
    out = {}
    for o, b in bufs.items():
        assert _untouched(b[:GUARD], o) and _untouched(b[GUARD + n:], o), f"{o}: an element outside the window was written"
        win = b[GUARD:GUARD + n]
        if expect == _lib.IKF_OK:
            written = ~torch.isnan(win) if o == "clearance" else win != _FILL[o]
            assert bool(written.all()), f"{o}: an element inside the window was not written"
        else:
            assert _untouched(win, o), f"{o}: a refused call wrote an output"
        out[o] = win.cpu().numpy().copy()
    return out


def _lattice_mask(eng, q, T, k, q_start=None, reject_self=False, self_min=0.0, stream=None, expect=_lib.IKF_OK):
    """ikf_sweep_lattice through eng.lib on a guarded buffer -> the words [T][k][ceil(k / 64)] uint64 (cpu numpy)."""
    words = (k + 63) // 64
    n = T * k * words
    sentinel = -0x5454545454545455   # 0xABAB... as int64
    buf = torch.full((n + 2 * GUARD,), sentinel, dtype=torch.int64, device=DEV)
    qd = q.to(DEV).contiguous()
    sd = None if q_start is None else q_start.to(DEV).contiguous()
    torch.cuda.synchronize()
    s = C.c_void_p(stream.cuda_stream) if stream is not None else C.c_void_p(0)
    code = eng.lib.ikf_sweep_lattice(eng._h, qd.data_ptr(), T, k, None if sd is None else sd.data_ptr(), int(reject_self), float(self_min),
                                     buf[GUARD:].data_ptr(), s)
    assert code == expect, (code, _lib.last_error(eng.lib))
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == sentinel).all()) and bool((buf[GUARD + n:] == sentinel).all()), "a word outside the window was written"
    if expect != _lib.IKF_OK:
        assert bool((buf[GUARD:GUARD + n] == sentinel).all()), "a refused call wrote a word"
    return buf[GUARD:GUARD + n].cpu().numpy().view(np.uint64).reshape(T, k, words)


def _unpack(words, T, k, with_start):
    """Mask words -> (edge_free [T][k][k] bool with row 0 all True, start_free [k] or None), as Engine.sweep_lattice returns them."""
    bits = ((words[..., None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool).reshape(T, k, -1)
    ef = bits[:, :, :k].copy()
    sf = bits[0, :, 0].copy() if with_start else None
    ef[0] = True
    return ef, sf


def _same(a, b):
    return all(PH.same_bits(a[n], b[n]) for n in OUTPUTS)


# ---- 1. off means off ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [False, True])
@pytest.mark.parametrize("sweep", [0, 4])
def test_search_without_a_track_after_a_cleared_one_and_under_a_far_one_is_the_same_call(sweep, world):
    """(65, 33) on the Panda: every output of ikf_path_search with no track, with a track set and then cleared, and with a track whose obstacles lie
    100 m away has the same bits - with and without a sweep, with and without a static world; the track in between does change the call."""
    T, k, which = 65, 33, "panda"
    L = SH.lattice_inputs(which, T, k, SH.LATTICE_SEEDS[(which, T, k)])
    eng = _eng(which)
    opt = _popt(max_step=2.0)
    eng.set_path_sweep(sweep)
    if world:
        eng.set_world(L["world"], L["world_thr"])
    plain = _path(eng, L["poses"], L["q"], k, opt, L["q_start"])
    assert eng.world_track_size == (0, 0)
    eng.set_world_track(TH.path_track(which, T, 0), TH.path_track_threshold(which, T, k, 0, L["q"]))
    assert eng.world_track_size == (T, 5)
    changed = _path(eng, L["poses"], L["q"], k, opt, L["q_start"])
    assert not PH.same_bits(changed["node"], plain["node"])
    assert (np.isposinf(plain["node"]) <= np.isposinf(changed["node"])).all()
    eng.clear_world_track()
    assert eng.world_track_size == (0, 0)
    assert _same(_path(eng, L["poses"], L["q"], k, opt, L["q_start"]), plain)
    eng.set_world_track(TH.far_track(T), 1.0)
    assert _same(_path(eng, L["poses"], L["q"], k, opt, L["q_start"]), plain)


def _tiny_solver():
    from ikflow_amd.ikflow_solver import IKFlowSolver

    robot, hp, lay, sd = H.tiny_model()   # (a robot of this test's own: the capsule model must not reach the solvers other modules share)
    robot.set_collision_capsules(RH.collision_capsules(robot))
    s = IKFlowSolver(hp, robot)
    s.load_state_dict_tensors(sd)
    return s, robot, lay


@pytest.mark.parametrize("sweep", [0, 4])
def test_generate_without_a_track_after_a_cleared_one_and_under_a_far_one_is_the_same_call(sweep):
    s, robot, lay = _tiny_solver()
    T, k = 33, 20
    poses = H.reachable_poses(robot, T, 11)[1].float()
    L = H.latents(k, lay.dim, 12)
    s.set_world(WH.scene("panda", SH.LATTICE_SCENE), 0.0)
    s.set_path_sweep(sweep)
    eng = s.engine(DEV)
    opt = _popt(limits=True)
    plain = _path(eng, poses, None, k, opt, latent=L)
    s.set_world_track(TH.moving_track("panda", T, "cheap5", 0), 0.05)
    assert eng.world_track_size == (T, 5)
    changed = _path(eng, poses, None, k, opt, latent=L)
    assert not PH.same_bits(changed["node"], plain["node"])
    s.set_world_track(None)
    assert eng.world_track_size == (0, 0)
    assert _same(_path(eng, poses, None, k, opt, latent=L), plain)
    s.set_world_track(TH.far_track(T), 1.0)
    assert _same(_path(eng, poses, None, k, opt, latent=L), plain)


# ---- 2. frames ---------------------------------------------------------------------------------------------------------------------------------------------
def test_frames_are_the_normalised_input_and_follow_the_sweep():
    """world_track_frame(t, 0) is the input as ikf_set_world normalises it, bit for bit, under every S; the fine frames are those of the S that is
    set - also after ikf_set_path_sweep changed it under a track - within one f32 ulp of the numpy fp64 restatement."""
    eng = _eng("panda")
    worlds = TH.moving_track("panda", 5, "mixed7", 0)
    kinds, keys = TH.stored_track(worlds)
    eng.set_world_track(worlds, 0.0)
    for S in (0, 3, 16, 1, 0):
        eng.set_path_sweep(S)
        ref = TH.interp_ref(kinds, keys, S)
        for t in range(5):
            for i in range(S + 1 if t < 4 else 1):
                got_kinds, got = TH.records_of(eng.world_track_frame(t, i))
                assert np.array_equal(got_kinds, kinds)
                if i == 0:
                    assert H.same_bits(got, keys[t]), f"S {S}: key frame {t} is not the normalised input"
                assert TH.ulp_excess(got, ref[TH.fine_index(t, i, S)]) <= 1.0, (S, t, i)
        for t, i in ((4, 1), (0, S + 1), (5, 0), (-1, 0), (0, -1)):
            with pytest.raises(EngineError, match="t must be in 0 .. F - 1 and i in 0 .. S"):
                eng.world_track_frame(t, i)
    eng.clear_world_track()
    with pytest.raises(EngineError, match="no track has been set"):
        eng.world_track_frame(0, 0)


# ---- 3. the node kernel against fp64 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,base,caps", TH.NODE_CASES, ids=lambda v: str(v))
def test_track_clearance_against_the_fp64_reference(which, base, caps, _small_model_back):
    """ikf_world_track_clearance on lattices of T = 1, 2, 5 waypoints and k = 1, 63, 64, 65 candidates - row r * T + t against key frame t - against
    world_helpers.reference on a World built from world_track_frame(t, 0): clearance within CLEARANCE_TOL, the closest pair the reference's unless
    its two best are within PAIR_AMBIGUITY, flags exact outside the band.  Every chain size on 7 obstacles of all four kinds; 1 and 64 obstacles and
    1 and 24 capsules on the Panda."""
    eng = _eng(which) if caps is None else _eng_model(which, caps, _small_model_back)
    c = TH.node_case(which, base, caps)
    kinds, keys = TH.stored_track(c["worlds"])
    eng.set_world_track(c["worlds"], c["thr"])
    assert eng.world_track_size == (TH.NODE_T, len(kinds))
    for t in range(TH.NODE_T):   # the reference's Worlds ARE those of world_track_frame(t, 0): the same numbers
        got_kinds, got = TH.records_of(eng.world_track_frame(t, 0))
        assert np.array_equal(got_kinds, kinds) and H.same_bits(got, keys[t])
    for T, k in TH.node_shapes(c):
        ref = {name: c["ref"][name][:k, :T].reshape(-1) for name in c["ref"]}
        assert not np.isnan(ref["clearance"]).any()
        out = _track_clearance(eng, TH.sub_lattice(c["q"], T, k), T, k)
        _check_against_reference(out, ref, c["thr"], k * T, f"{which} {base} {caps} T {T} k {k}")
    assert 0 < out["colliding"].sum() < out["colliding"].size or out["colliding"].size < 5


# ---- 4. the sweep mask against fp64 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_start", [True, False])
@pytest.mark.parametrize("case", TH.MASK_CASES, ids=lambda c: "-".join(map(str, c)))
def test_sweep_lattice_against_the_fp64_reference(case, with_start):
    """ikf_sweep_lattice under the track alone, track + the static scene mixed7, and both with the self rule: the verdict of every edge - sample i of
    the edge into waypoint t against a World from world_track_frame(t - 1, i), the start edges against key frame 0 - is the reference's outside the
    band.  Thresholds: per rule the median over the edges of the minimum over their samples; the seed satisfies sweep_helpers.shares_hold."""
    T, k, S, rule, base = case
    seed = TH.mask_seed(*case)
    eng = _eng(TH.MASK_CHAIN)
    q, q_start, worlds = TH.mask_inputs(T, k, S, base, seed)
    eng.set_path_sweep(S)
    eng.set_world_track(worlds, 0.0)
    c = TH.mask_case(T, k, S, rule, base, seed, frames=eng.world_track_frame)
    v = c["v"] if with_start else c["v_nostart"]
    band, blocked, free = SH.shares(v)
    print(f"{case} start {with_start}: band {band:.4f} (cap 0.02), surely blocked {blocked:.3f}, surely free {free:.3f}")
    assert SH.shares_hold(v), (case, SH.shares(v))
    eng.set_world_track(worlds, c["track_thr"])
    if c["world"] is not None:
        eng.set_world(c["world"], c["world_thr"])
    ef, sf = eng.sweep_lattice(q.to(DEV), T, k, q_start.to(DEV) if with_start else None, reject_self=rule == "all", min_clearance=c["self_thr"] or 0.0)
    assert ef.dtype == torch.bool and ef.shape == (T, k, k) and bool(ef[0].all())
    assert (sf is None) == (not with_start) and (sf is None or (sf.dtype == torch.bool and sf.shape == (k,)))
    free_bits = ef[1:].reshape(-1).cpu().numpy()
    if with_start:
        free_bits = np.concatenate([free_bits, sf.cpu().numpy()])
    sure = ~v["band"]
    bad = sure & (~free_bits != v["blocked"])
    assert not bad.any(), f"{case}: {int(bad.sum())} verdicts differ from the fp64 reference outside the band, first {np.flatnonzero(bad)[:5]}"
    assert 0 < (~free_bits).sum() < free_bits.size
    # the raw entry on a guarded buffer gives the same words, and padding bits of the last word are never set
    words = _lattice_mask(eng, q, T, k, q_start if with_start else None, rule == "all", c["self_thr"] or 0.0)
    ef2, sf2 = _unpack(words, T, k, with_start)
    assert np.array_equal(ef2, ef.cpu().numpy()) and (sf2 is None or np.array_equal(sf2, sf.cpu().numpy()))
    if k % 64:
        assert not (words[1:, :, -1] >> np.uint64(k % 64)).any()


# ---- 5. the path equals its parts, bit for bit ------------------------------------------------------------------------------------------------------------------
PARTS_SHAPES = {"panda": (65, 33, "panda"), "fetch": (65, 33, "fetch"), "syn5p": (65, 33, "syn5p"), "T3_k129": (3, 129, "panda"), "T5_k256": (5, 256, "panda")}
PARTS_VARIANTS = ("plain", "step_gate", "self_rule", "cloud", "no_sweep")


@pytest.mark.parametrize("variant", PARTS_VARIANTS)
@pytest.mark.parametrize("shape", list(PARTS_SHAPES))
def test_path_search_under_a_track_equals_its_parts(shape, variant):
    """ikf_path_search with a static world, a sweep and a track == sweep_helpers.dp_f32_masked on (node costs: ikf_rank_candidates' row scores with
    +inf where ikf_world_track_clearance < the track's threshold; mask: ikf_sweep_lattice): node costs, path, index, cost and reachable_out, bit
    for bit - with q_start, with a step gate, with the self rule, with a cloud set as well, and with no sweep (nodes only)."""
    T, k, which = PARTS_SHAPES[shape]
    seed = SH.SELF_RULE_SEED if (variant == "self_rule" and which == "panda" and T == 65) else SH.LATTICE_SEEDS.get((which, T, k), 0)
    L = SH.lattice_inputs(which, T, k, seed)
    eng = _eng(which)
    S = 0 if variant == "no_sweep" else 4
    eng.set_world(L["world"], L["world_thr"])
    eng.set_path_sweep(S)
    thr = TH.path_track_threshold(which, T, k, 0, L["q"])
    eng.set_world_track(TH.path_track(which, T, 0), thr)
    if variant == "cloud":
        pts = CH.cloud(which, 511)
        eng.set_world_cloud(pts, CH.POINT_RADIUS, 0.0)
        # not an accuracy claim: only a threshold that rejects about a tenth of these rows
        eng.set_world_cloud(pts, CH.POINT_RADIUS, float(torch.quantile(eng.cloud_clearance(L["q"].to(DEV))[0], 0.1)))
    opt = _popt(max_step=SH.STEP_GATE if variant == "step_gate" else None, collisions=variant == "self_rule",
                min_clearance=L["self_thr"] if variant == "self_rule" else 0.0)
    q_start = L["q_start"]
    out = _path(eng, L["poses"], L["q"], k, opt, q_start)
    scores = _rank(eng, L["poses"], L["q"], k, _rank_opt(1, opt.rot_weight, 0.0, None, None, False, bool(opt.reject_collisions), opt.min_clearance))["row_score"]
    tc = _track_clearance(eng, L["q"], T, k)
    node = np.where(tc["clearance"] < np.float32(thr), INF, scores.reshape(-1)).astype(np.float32)
    assert np.array_equal(tc["colliding"].astype(bool), tc["clearance"] < np.float32(thr))
    assert PH.same_bits(out["node"], node), "node costs are not the ranking's row scores with +inf where the track rejects"
    masked = int((np.isposinf(node) & ~np.isposinf(scores.reshape(-1))).sum())
    assert masked > 0, "the track rejects no row the ranking admits: the case does not test the node sink"
    if S:
        ef, sf = eng.sweep_lattice(L["q"].to(DEV), T, k, q_start.to(DEV), reject_self=bool(opt.reject_collisions), min_clearance=opt.min_clearance)
        ef, sf = ef.cpu().numpy(), sf.cpu().numpy()
    else:
        with pytest.raises(EngineError, match="no sweep is set"):
            eng.sweep_lattice(L["q"].to(DEV), T, k)
        ef, sf = None, None
    _check_against_masked_dp(out, L["q"], T, k, opt, ef, sf, q_start, f"{shape} {variant}")
    if S:
        nb, nf = _admissible_edge_counts(out["node"], ef, sf, T, k)
        print(f"{shape} {variant}: {masked} rows masked by the track, {nb} blocked and {nf} free edges between admissible nodes")
        assert nb > 0 and nf > 0
        # the track does block edges the static rules leave free
        eng.clear_world_track()
        ef0, sf0 = eng.sweep_lattice(L["q"].to(DEV), T, k, q_start.to(DEV), reject_self=bool(opt.reject_collisions), min_clearance=opt.min_clearance)
        assert int((~ef[1:]).sum()) > int((~ef0.cpu().numpy()[1:]).sum())


@pytest.mark.parametrize("shared", [True, False])
def test_generate_path_under_a_track_equals_the_flow_then_path_search(shared):
    s, robot, lay = _tiny_solver()
    T, k, S = 33, 20, 4
    poses = H.reachable_poses(robot, T, 11)[1].float()
    L = H.latents(k if shared else k * T, lay.dim, 12)
    expanded = L[:, None, :].expand(k, T, lay.dim).reshape(k * T, lay.dim).contiguous() if shared else L
    rows = s.generate_ik_solutions(poses.to(DEV).repeat((k, 1)), latent=expanded.to(DEV))
    worlds = TH.moving_track("panda", T, "cheap5", 0)
    s.set_world_track(worlds, 0.0)
    eng = s.engine(DEV)
    # not an accuracy claim: only a threshold that rejects about a quarter of these rows
    thr = float(torch.quantile(eng.world_track_clearance(rows, T, k)[0], 0.25))
    s.set_world_track(worlds, thr)
    s.set_path_sweep(S)
    opt = _popt(limits=True)
    one = _path(eng, poses, None, k, opt, latent=L, shared=shared)
    two = _path(eng, poses, rows.cpu(), k, opt)
    assert _same(one, two)
    ef, sf = eng.sweep_lattice(rows, T, k)
    _check_against_masked_dp(one, rows.cpu(), T, k, opt, ef.cpu().numpy(), None, None, f"tiny shared {shared}")
    assert 0 < np.isposinf(one["node"]).sum() < k * T
    nb, nf = _admissible_edge_counts(one["node"], ef.cpu().numpy(), None, T, k)
    assert nb > 0 and nf > 0


# ---- 6. the obstacle really moves -----------------------------------------------------------------------------------------------------------------------------
def test_an_obstacle_that_crosses_an_edge_between_two_key_frames_blocks_that_edge_alone():
    """T = 3, k = 3, S = 1: the sphere is on the middle sample of the edge (0, 0) -> (1, 0) in fine frame (0, 1) only.  Under each key frame as a static
    world every edge is free and the path is candidate 0 throughout; under the track exactly that edge is blocked, every node stays admissible,
    and the path avoids the edge and costs more."""
    c = TH.moving_crossing_case("edge")
    eng = _eng("panda")
    opt = _popt()
    q = c["q"]
    eng.set_path_sweep(1)
    for key in c["worlds"]:
        eng.set_world(key, 0.0)
        ef, _ = eng.sweep_lattice(q.to(DEV), 3, 3)
        assert bool(ef.all())
        static = _path(eng, c["poses"], q, 3, opt)
        assert list(static["index"]) == [0, 0, 0] and np.isfinite(static["node"]).all()
    eng.clear_world()
    eng.set_world_track(c["worlds"], 0.0)
    ef, _ = eng.sweep_lattice(q.to(DEV), 3, 3)
    ef = ef.cpu().numpy()
    assert not ef[1, 0, 0] and int((~ef).sum()) == 1, ef
    out = _path(eng, c["poses"], q, 3, opt)
    assert PH.same_bits(out["node"], static["node"]) and np.isfinite(out["cost"][0])
    assert not (out["index"][0] == 0 and out["index"][1] == 0) and out["cost"][0] > static["cost"][0]
    assert list(out["reach"]) == [3, 3, 3]


def test_an_obstacle_that_sits_on_a_node_in_its_own_key_frame_only_takes_that_node_away():
    """The sphere is on candidate 0 of waypoint 1 in key frame 1 and far away in key frames 0 and 2: that node alone costs +inf (with and without a
    sweep), no edge between admissible nodes is blocked, and the path goes round the node and costs more."""
    c = TH.moving_crossing_case("node")
    eng = _eng("panda")
    opt = _popt()
    q = c["q"]
    base = _path(eng, c["poses"], q, 3, opt)
    assert list(base["index"]) == [0, 0, 0]
    for S in (0, 1):
        eng.set_path_sweep(S)
        eng.set_world_track(c["worlds"], 0.0)
        out = _path(eng, c["poses"], q, 3, opt)
        want = base["node"].copy()
        want[0 * 3 + 1] = INF
        assert PH.same_bits(out["node"], want)
        assert out["index"][1] != 0 and np.isfinite(out["cost"][0]) and out["cost"][0] > base["cost"][0]
        assert list(out["reach"]) == [3, 2, 3]
    ef, _ = eng.sweep_lattice(q.to(DEV), 3, 3)
    assert bool(ef.all())
    tc = _track_clearance(eng, q, 3, 3)
    assert list(np.flatnonzero(tc["colliding"])) == [1] and tc["obstacle"][1] == 0


# ---- 7. edges of the interface ---------------------------------------------------------------------------------------------------------------------------------
def _obstacles(worlds):
    flat = [o for w in worlds for o in w.obstacles]
    arr = (_lib.ikf_obstacle * len(flat))()
    for o, (kind, a, b, quat, radius) in zip(arr, flat):
        o.kind, o.radius = int(kind), float(radius)
        for i in range(3):
            o.a[i], o.b[i] = float(a[i]), float(b[i])
        for i in range(4):
            o.quat[i] = float(quat[i])
    return arr


def test_refusals_keep_the_old_track_and_name_frame_and_obstacle():
    from ikflow_amd.engine import Engine
    from ikflow_amd.world import World

    which, T, k = "panda", 5, 8
    eng = _eng(which)
    lib = eng.lib
    q, q_start, worlds = TH.mask_inputs(T, k, 3, "mixed7", 0)
    opt = _popt()
    poses = torch.zeros(T, 7)
    poses[:, 3] = 1.0
    eng.set_path_sweep(3)
    eng.set_world_track(worlds, 0.05)
    before = _track_clearance(eng, q, T, k)
    mask_before = _lattice_mask(eng, q, T, k, q_start)

    def still_the_old_track():
        assert eng.world_track_size == (T, 7)
        assert all(H.same_bits(v, before[o]) for o, v in _track_clearance(eng, q, T, k).items())
        assert H.same_bits(_lattice_mask(eng, q, T, k, q_start), mask_before)

    arr = _obstacles(worlds)
    bad = _obstacles(worlds)
    bad[3 * 7 + 2].kind = 0                                      # frame 3 obstacle 2: a half-space becomes a sphere
    assert lib.ikf_set_world_track(eng._h, bad, T, 7, 0.0) == _lib.IKF_ERR_BAD_ARGUMENT
    assert "frame 3 obstacle 2: kind 0 differs from frame 0's kind 2" in _lib.last_error(lib)
    still_the_old_track()
    bad = _obstacles(worlds)
    bad[4 * 7 + 0].radius = -1.0
    assert lib.ikf_set_world_track(eng._h, bad, T, 7, 0.0) == _lib.IKF_ERR_BAD_ARGUMENT and "frame 4 obstacle 0: radius must be >= 0" in _lib.last_error(lib)
    bad = _obstacles(worlds)
    bad[1 * 7 + 3].b[1] = 0.0
    assert lib.ikf_set_world_track(eng._h, bad, T, 7, 0.0) == _lib.IKF_ERR_BAD_ARGUMENT and "frame 1 obstacle 3: half extents must be > 0" in _lib.last_error(lib)
    bad = _obstacles(worlds)
    bad[2 * 7 + 2].a[0] = bad[2 * 7 + 2].a[1] = bad[2 * 7 + 2].a[2] = 0.0
    assert lib.ikf_set_world_track(eng._h, bad, T, 7, 0.0) == _lib.IKF_ERR_BAD_ARGUMENT and "frame 2 obstacle 2: zero normal" in _lib.last_error(lib)
    bad = _obstacles(worlds)
    bad[0].a[2] = float("nan")
    assert lib.ikf_set_world_track(eng._h, bad, T, 7, 0.0) == _lib.IKF_ERR_BAD_ARGUMENT and "frame 0 obstacle 0: non-finite number" in _lib.last_error(lib)
    for n_frames, n_obs, msg in ((T, 0, "n_obstacles must be in 1 .. 64"), (T, 65, "n_obstacles must be in 1 .. 64"), (1025, 7, "n_frames must be in 0 .. 1024"),
                                 (-1, 7, "n_frames must be in 0 .. 1024")):
        assert lib.ikf_set_world_track(eng._h, arr, n_frames, n_obs, 0.0) == _lib.IKF_ERR_BAD_ARGUMENT and msg in _lib.last_error(lib)
    assert lib.ikf_set_world_track(eng._h, arr, T, 7, float("nan")) == _lib.IKF_ERR_BAD_ARGUMENT and "min_clearance must be finite" in _lib.last_error(lib)
    assert lib.ikf_set_world_track(eng._h, None, T, 7, 0.0) == _lib.IKF_ERR_NULL_POINTER
    still_the_old_track()
    # opposite normals in consecutive frames: the blend at u = 1 / 2 vanishes - refused under S = 3, by the set and by a change of the sweep
    flip = []
    for t in range(3):
        w = World()
        w.add_half_space((0.0, 0.0, 1.0) if t < 2 else (0.0, 0.0, -1.0), -5.0)
        flip.append(w)
    with pytest.raises(EngineError, match="frame 1 obstacle 0: the normal blended with frame 2's at sample 2 of 3 is shorter than 1e-6"):
        eng.set_world_track(flip, 0.0)
    still_the_old_track()
    eng.set_path_sweep(2)
    eng.set_world_track(flip, 0.0)                                # u = 1 / 3, 2 / 3: fine
    with pytest.raises(EngineError, match="ikf_set_path_sweep: frame 1 obstacle 0"):
        eng.set_path_sweep(1)
    assert eng.path_sweep == 2 and eng.world_track_size == (3, 1)
    eng.set_world_track(worlds, 0.05)
    eng.set_path_sweep(3)
    still_the_old_track()
    # T > F is refused before anything is written, T < F is accepted
    q6, _, _ = TH.mask_inputs(T + 1, k, 3, "mixed7", 0)
    poses6 = torch.zeros(T + 1, 7)
    poses6[:, 3] = 1.0
    with pytest.raises(EngineError, match="ikf_path_search: T = 6 waypoints, but the world track has 5 frames"):
        eng.path_search(poses6.to(DEV), k, q6.to(DEV), opt)
    _track_clearance(eng, q6, T + 1, k, expect=_lib.IKF_ERR_BAD_ARGUMENT)
    _lattice_mask(eng, q6, T + 1, k, expect=_lib.IKF_ERR_BAD_ARGUMENT)
    assert "ikf_sweep_lattice: T = 6 waypoints" in _lib.last_error(lib)
    q3 = q.reshape(k, T, -1)[:, :3].reshape(3 * k, -1).contiguous()   # waypoints 0 .. 2 of the same lattice
    short = _path(eng, poses[:3], q3, k, opt)
    tc3 = _track_clearance(eng, q3, 3, k)
    assert H.same_bits(tc3["clearance"], before["clearance"].reshape(k, T)[:, :3].reshape(-1))
    assert np.array_equal(np.isposinf(short["node"]), tc3["colliding"].astype(bool))
    eng.set_world_track(worlds[:3], 0.05)                         # the same three key frames as a track of their own: the same clearances
    assert H.same_bits(_track_clearance(eng, q3, 3, k)["clearance"], tc3["clearance"])
    eng.set_world_track(worlds, 0.05)
    # nullable outputs, a side stream, k out of range, S = 0, no track, no collision model
    for null in (("clearance",), ("obstacle", "capsule"), ("colliding",), CLEARANCE_OUTPUTS):
        got = _track_clearance(eng, q, T, k, null=null)
        assert all(H.same_bits(v, before[o]) for o, v in got.items())
    side = torch.cuda.Stream(device=DEV)
    assert all(H.same_bits(v, before[o]) for o, v in _track_clearance(eng, q, T, k, stream=side).items())
    assert H.same_bits(_lattice_mask(eng, q, T, k, q_start, stream=side), mask_before)
    main = _path(eng, poses, q, k, opt, q_start)
    assert _same(_path(eng, poses, q, k, opt, q_start, stream=side), main)
    for bad_k in (0, 257):
        assert lib.ikf_sweep_lattice(eng._h, 1, T, bad_k, None, 0, 0.0, 1, None) == _lib.IKF_ERR_BAD_ARGUMENT and "k must be in 1 .. 256" in _lib.last_error(lib)
    assert lib.ikf_sweep_lattice(eng._h, None, T, k, None, 0, 0.0, None, None) == _lib.IKF_ERR_NULL_POINTER
    assert lib.ikf_sweep_lattice(eng._h, None, 0, k, None, 0, 0.0, None, None) == _lib.IKF_OK            # T = 0: nothing to do
    eng.set_path_sweep(0)
    _lattice_mask(eng, q, T, k, expect=_lib.IKF_ERR_BAD_ARGUMENT)
    assert "no sweep is set" in _lib.last_error(lib)
    eng.clear_world_track()
    _track_clearance(eng, q, T, k, expect=_lib.IKF_ERR_BAD_ARGUMENT)
    assert "no track has been set" in _lib.last_error(lib)
    fresh = Engine(eng.layout, eng.robot, DEV)   # no collision model
    assert lib.ikf_set_world_track(fresh._h, arr, T, 7, 0.0) == _lib.IKF_ERR_BAD_ARGUMENT and "without a collision model" in _lib.last_error(lib)
    assert fresh.world_track_size == (0, 0)
    fresh.clear_world_track()                                     # clearing needs nothing


def test_after_reserve_path_a_call_under_a_track_allocates_nothing():
    """The method of tests/test_sweep.py::test_after_set_path_sweep_and_reserve_path_a_call_of_that_size_allocates_nothing, with a track on the handle:
    ikf_generate_path, ikf_world_track_clearance and ikf_sweep_lattice of the reserved size and below."""
    from ikflow_amd.engine import Engine

    s, robot, lay = _tiny_solver()
    T, k = 300, 64
    poses = H.reachable_poses(robot, T, 3)[1].float()
    Lk = H.latents(k, lay.dim, 5)
    opt = _popt(limits=True)
    worlds = TH.moving_track("panda", T, "cheap5", 0)

    def engine():
        eng = Engine(s.layout, robot, DEV)
        eng.load_state_dict(s._state_dict_np)
        eng.set_collision_model(*robot._collision_model)
        eng.set_path_sweep(2)
        eng.set_world_track(worlds, 0.02)
        return eng

    rows = torch.zeros(T * k, robot.ndof, device=DEV)

    def run(eng, tt, kk):
        out = _path(eng, poses[:tt], None, kk, opt, latent=Lk[:kk], shared=True)
        _track_clearance(eng, rows[:tt * kk], tt, kk)
        _lattice_mask(eng, rows[:tt * kk], tt, kk)
        return out

    eng = engine()
    eng.reserve_path(T, k)
    torch.cuda.synchronize()
    run(eng, 8, 4)                                                     # (torch's caching allocator warm for the test's own buffers)
    run(eng, T, k)
    torch.cuda.synchronize()
    free0, stat0 = torch.cuda.mem_get_info(DEV)[0], torch.cuda.memory_reserved(DEV)
    full = run(eng, T, k)
    run(eng, 100, 50)
    run(eng, 1, 64)
    torch.cuda.synchronize()
    free1, stat1 = torch.cuda.mem_get_info(DEV)[0], torch.cuda.memory_reserved(DEV)
    grown_by_torch = stat1 - stat0
    assert free0 - free1 <= grown_by_torch, f"the engine allocated {free0 - free1 - grown_by_torch} bytes after ikf_reserve_path under a track"
    fresh = engine()
    assert all(PH.same_bits(full[n], v) for n, v in run(fresh, T, k).items())   # (the reservation changes no result)


def test_a_track_on_one_handle_does_not_change_another():
    from ikflow_amd.engine import Engine

    T, k, which = 65, 33, "panda"
    L = SH.lattice_inputs(which, T, k, SH.LATTICE_SEEDS[(which, T, k)])
    robot, _ = H.kin_robots(which)
    eng = _eng(which)
    other = Engine(eng.layout, eng.robot, DEV)
    other.set_collision_model(*robot._collision_model)
    opt = _popt()
    for e in (eng, other):
        e.set_path_sweep(4)
    plain = _path(other, L["poses"], L["q"], k, opt)
    thr = TH.path_track_threshold(which, T, k, 0, L["q"])
    eng.set_world_track(TH.path_track(which, T, 0), thr)
    other.set_world_track(TH.moving_track(which, T, "one", 3), 0.1)
    assert eng.world_track_size == (T, 5) and other.world_track_size == (T, 1)
    a, b = _path(eng, L["poses"], L["q"], k, opt), _path(other, L["poses"], L["q"], k, opt)
    assert not PH.same_bits(a["node"], b["node"]) and not PH.same_bits(b["node"], plain["node"])
    other.clear_world_track()
    assert eng.world_track_size == (T, 5)
    assert _same(_path(eng, L["poses"], L["q"], k, opt), a) and _same(_path(other, L["poses"], L["q"], k, opt), plain)


def test_python_wrappers_and_a_solver_set_before_its_engine_exists():
    """IKFlowSolver.set_world_track before the first GPU call is remembered and pushed, after the collision model, the world and the sweep, to the
    engine the solver creates; generate_ik_path keeps its signature and honours the track; timed_path_collides is sweep_lattice at k = 1."""
    s, robot, lay = _tiny_solver()
    T, k, S = 33, 20, 3
    worlds = TH.moving_track("panda", T, "cheap5", 0)
    assert s._engine is None
    s.set_path_sweep(S)                    # no engine yet: remembered
    s.set_world_track(worlds, 0.03)        # creates the solver's engine and pushes collision model, sweep and track to it
    eng = s.engine(DEV)
    assert eng.path_sweep == S and eng.world_track_size == (T, 5) and eng.has_collision_model
    kinds, keys = TH.stored_track(worlds)
    assert H.same_bits(TH.records_of(eng.world_track_frame(7, 0))[1], keys[7])
    s.set_world_track(worlds[:T - 1], 0.03)
    assert eng.world_track_size == (T - 1, 5)
    w = H.reachable_poses(robot, T, 21)[1].float().to(DEV)
    Lk = H.latents(k, lay.dim, 22).to(DEV)
    with pytest.raises(EngineError, match="T = 33 waypoints, but the world track has 32 frames"):
        s.generate_ik_path(w, k, latent=Lk, reject_self_collisions=False)
    s.set_world_track(None)
    a = s.generate_ik_path(w, k, latent=Lk, reject_self_collisions=False, return_node_costs=True)
    s.set_world_track(worlds, 0.03)
    b = s.generate_ik_path(w, k, latent=Lk, reject_self_collisions=False, return_node_costs=True)
    assert a._fields == b._fields and bool((torch.isinf(a.node_costs) <= torch.isinf(b.node_costs)).all())
    assert int(torch.isinf(b.node_costs).sum()) > int(torch.isinf(a.node_costs).sum())
    # timed_path_collides == sweep_lattice at k = 1, with and without q_start; a returned path that exists is free by it
    rows = s.generate_ik_solutions(w, latent=Lk[:1].expand(T, lay.dim).contiguous())
    q_start = rows[0] + 0.05
    for start in (None, q_start):
        flags = s.timed_path_collides(rows, start)
        ef, sf = eng.sweep_lattice(rows, T, 1, start)
        assert flags.dtype == torch.bool and flags.shape == (T,)
        assert torch.equal(flags[1:], ~ef[1:, 0, 0]) and bool(flags[0]) == (False if sf is None else not bool(sf[0]))
    if bool(torch.isfinite(b.cost)):
        assert not bool(s.timed_path_collides(b.path).any())
    assert s.timed_path_collides(rows[:0]).shape == (0,)
    tc = eng.world_track_clearance(rows, T, 1)
    assert tc[0].dtype == torch.float32 and tc[1].dtype == torch.int32 and tc[3].dtype == torch.bool and tc[0].shape == (T,)
    assert torch.equal(tc[3], tc[0] < 0.03)
    s.set_world_track(None)
    s.set_path_sweep(0)
