"""CPU-side checks of flow chaining: the float64 restatement the GPU tests compare with (tests/chain_ref.py) on scenes whose answer
is known in closed form, its own fp32 error (the measured base of the GPU tolerances), the conditions the GPU test's cases have to
meet, the argument validation of ofd_flow_chain, ofd_flow_chain_to and ofd_layer_composite, which happens before any HIP call, and the
host logic of warp.chain_flows, warp.chain_flows_to, warp.composite_layer and FlowDiffuser.estimate_flow_clip / track / propagate."""
import ctypes

import pytest
import torch

import chain_ref as R
from test_constrained_sampling_cpu import host_registry          # noqa: F401 (fixture: the plugins construct without a GPU)


@pytest.fixture(scope="module")
def lib():
    from opticalflowdiffusion_amd import build, _lib
    build.build(verbose=False)
    return _lib.lib()


# ---------------------------------------------------------------------------------------------------------------------- restatement
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
def test_moving_rectangle_tracks_are_the_closed_form(dtype):
    """a rectangle moving by (5, -3) per frame over a still background, true flows, 19 x 70, T = 3: a background pixel dies
    `inconsistent` on arrival at the first frame where the rectangle covers it, a rectangle pixel dies `leaves` at the first step that
    takes it outside, everything else is tracked with D = i * move (0 for the background).  Per frame 61 / 122 / 171 pixels are
    inconsistent and 12 have left at frame 3 (the rectangle's top row, which reaches y = -1).  Without the check nothing is ever
    inconsistent."""
    H, W, T, rect = 19, 70, 3, R.RECT_19x70
    fwd, bwd = R.rect_clip(H, W, [rect], T)
    r = R.chain_ref(fwd, bwd, 0, T, True, dtype=dtype)
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    on = R.rect_mask(H, W, rect, 0)
    want_state = torch.zeros(T + 1, H, W, dtype=torch.long)
    want_disp = torch.zeros(T + 1, 2, H, W, dtype=dtype)
    dead = torch.zeros(H, W, dtype=torch.bool)
    for i in range(1, T + 1):
        gone = on & ~dead & ((xs + i * R.MOVE[0] > W - 1) | (ys + i * R.MOVE[1] < 0))
        covered = ~on & ~dead & R.rect_mask(H, W, rect, i)
        want_state[i] = want_state[i - 1]
        want_state[i][gone], want_state[i][covered] = R.LEAVES, R.INCONSISTENT
        dead = dead | gone | covered
        for c in range(2):
            want_disp[i, c][on] = float(i * R.MOVE[c])
        want_disp[i][:, dead] = float("nan")
    got_state, got_disp = r["state"][0, :, 0].long(), r["disp"][0]
    assert torch.equal(got_state, want_state)
    assert torch.equal(torch.isnan(got_disp), torch.isnan(want_disp)) and torch.equal(got_disp.nan_to_num(), want_disp.nan_to_num())
    assert [int((got_state[i] == R.INCONSISTENT).sum()) for i in range(T + 1)] == [0, 61, 122, 171]
    assert [int((got_state[i] == R.LEAVES).sum()) for i in range(T + 1)] == [0, 0, 0, 12]
    life = r["life"][0, 0]
    assert torch.equal(life, (got_state == R.TRACKED)[1:].sum(0).to(torch.int32)) and int(life.min()) == 0 and int(life.max()) == T
    free = R.chain_ref(fwd, bwd, 0, T, False, dtype=dtype)
    # (a covered background pixel then lives on, is picked up by the rectangle one frame later and may leave with it)
    assert not (free["state"] == R.INCONSISTENT).any() and int((free["state"][0, -1] == R.LEAVES).sum()) >= 12
    assert torch.isnan(free["margin"]).all()
    # n = 0: slot 0 alone
    still = R.chain_ref(fwd, bwd, 2, 2, True, dtype=dtype)
    assert still["disp"].shape == (1, 1, 2, H, W) and not still["disp"].any() and not still["state"].any() and not still["life"].any()


def test_rotation_composes_where_summing_drifts():
    """six rotations about the centre of a 33 x 129 frame: the composed track is the closed form R^j p - p (the fields are linear in p,
    so the bilinear read is exact; measured 3.4e-7 px, the fp32 rounding of the fields), the sum of the fields at the fixed pixel is
    off by more than a pixel (measured: maximum 1.35, mean 0.64 over the living tracks at the last frame), and about three
    quarters of the tracks live to the end (measured 74.96 %)."""
    r = R.walk_ref("33x129-rotation", 0, 6, True)
    closed = R.rotation_closed_form()
    alive = ~torch.isnan(r["disp"][0])
    assert torch.equal(alive[:, 0], r["state"][0, :, 0] == R.TRACKED)
    err = float((r["disp"][0] - closed)[alive].abs().max())
    fwd, _bwd = R.make_case("33x129-rotation")
    naive = torch.cumsum(fwd[0].double(), 0)
    off = (naive - closed[1:]).pow(2).sum(1).sqrt()[-1][alive[-1, 0]]
    share = float(alive[-1, 0].float().mean())
    print(f"rotation: composed vs closed form {err:.3e} px, naive sum off by max {float(off.max()):.3f} mean {float(off.mean()):.3f} px, "
          f"{share:.2%} live to the end")
    assert err <= 1e-5 and float(off.max()) > 1.0 and 0.7 <= share <= 0.8
    assert not (r["state"] == R.INCONSISTENT).any()                         # true inverse flows: every round trip closes
    dead = r["state"][0, -1, 0] != R.TRACKED
    assert torch.equal(dead, r["state"][0, -1, 0] == R.LEAVES)


@pytest.mark.parametrize("name", [n for n, c in R.CASES.items() if not c[4]])
def test_conditioning_is_at_or_below_the_pinned_values(name):
    """max |fp32 run - fp64 run| of the restatement over every walk of the case.  Measured: rotation 2.182e-6 px on D and 1.720e-7 on
    e2 - bound, 19x70 smooth 1.429e-6 and 3.451e-6, 33x129 smooth 1.346e-6 and 3.254e-6."""
    dD, dM = R.conditioning(name)
    print(f"{name}: max |fp32 - fp64|  D {dD:.3e}  e2 - bound {dM:.3e}")
    assert dD <= R.PINNED[name][0] and dM <= R.PINNED[name][1]
    assert R.PINNED[name][0] <= 1.4 * dD and R.PINNED[name][1] <= 1.4 * dM            # and the table is the measurement, not a guess


@pytest.mark.parametrize("run", R.RUNS, ids=lambda r: "-".join(str(v) for v in r))
def test_restatement_fp32_run_and_left_out_cap(run):
    """the fp32 run of the restatement against its float64 run, per run of the GPU test.  Exact cases: the same bits in every output.
    Inexact cases: the left-out set stays under the cap (measured: no entry in any run as the cases stand), outside it both runs give the
    same states and D differs by at most the pinned value; the smooth cases have `tracked` and `inconsistent` both well populated."""
    name, kind, a, b, check = run
    exact = R.CASES[name][4]
    if kind == "walk":
        r64, r32 = R.walk_ref(name, a, b, check), R.walk_ref(name, a, b, check, torch.float32)
        d64, s64, d32, s32, out = r64["disp"], r64["state"], r32["disp"], r32["state"], R.left_out_walk(name, a, b, check)
    else:
        d64, s64, out = R.to_ref(name, a, check)
        d32, s32, _ = R.to_ref(name, a, check, torch.float32)
    share = float(out.float().mean())
    print(f"{run}: left out {share:.3%}, final states {[int((s64[:, -1] == k).sum()) for k in range(6)]}")
    assert share <= R.LEFT_OUT_CAP                                          # a condition on the case: change its field, never the cap
    if exact:
        assert not out.any() and torch.equal(s32, s64)
        assert torch.equal(torch.isnan(d32), torch.isnan(d64)) and torch.equal(d32.nan_to_num().view(torch.int32), d64.float().nan_to_num().view(torch.int32))
        if kind == "walk":
            assert torch.equal(r32["life"], r64["life"])
        return
    keep = ~out
    assert torch.equal(s32[keep], s64[keep])
    keep2 = keep.expand(-1, -1, 2, -1, -1)
    assert torch.equal(torch.isnan(d32[keep2]), torch.isnan(d64[keep2]))
    assert float((d32.double() - d64)[keep2].nan_to_num().abs().max()) <= R.PINNED[name][0]
    if "smooth" in name and check and kind == "walk":
        total = s64[:, -1].numel()
        assert int((s64[:, -1] == R.TRACKED).sum()) >= 0.1 * total and int((s64[:, -1] == R.INCONSISTENT).sum()) >= 0.3 * total


def test_special_values_take_the_states_the_header_names():
    ahead, back = R.walk_ref("16x24-special", 0, 2, True), R.walk_ref("16x24-special", 2, 0, True)
    s, d, life = ahead["state"][0, :, 0], ahead["disp"][0], ahead["life"][0, 0]
    at = lambda t, pts: [int(t[y, x]) for y, x in pts]
    assert at(s[1], ((3, 4), (3, 3), (2, 4), (2, 3))) == [R.INVALID] * 4              # a NaN corner of the stepping field, also under weight 0
    assert at(s[1], ((5, 6), (5, 5), (4, 6), (4, 5))) == [R.INVALID] * 4              # +inf likewise
    assert at(s[1], ((10, 10), (4, 17))) == [R.LEAVES] * 2                            # 1e30, and one past the border
    assert at(s[1], ((8, 8), (8, 7), (7, 8), (7, 7))) == [R.UNMATCHED] * 4            # -inf in the checking field, also under weight 0
    assert at(s[1], ((10, 9), (9, 10), (9, 9))) == [R.UNMATCHED] * 3
    assert at(s[1], ((9, 2),)) == [R.INCONSISTENT]
    assert at(s[2], ((2, 15), (6, 1), (7, 0), (13, 5))) == [R.TRACKED] * 4            # q' on W - 1, H - 1 and 0 is inside; -0.0
    assert d[2, :, 2, 15].tolist() == [8.0, 0.0] and d[2, :, 6, 1].tolist() == [0.0, 9.0] and d[2, :, 13, 5].tolist() == [-5.0, 0.0]
    assert at(s[1], ((12, 20),)) == [R.TRACKED] and at(s[2], ((12, 20),)) == [R.INVALID] and int(life[12, 20]) == 1
    assert torch.equal(s[2][s[1] != R.TRACKED], s[1][s[1] != R.TRACKED])              # a dead track keeps its state
    assert torch.isnan(d[2][:, s[1] != R.TRACKED]).all() and torch.equal(torch.isnan(d[:, 0]), s != R.TRACKED)
    sb, db = back["state"][0, :, 0], back["disp"][0]
    assert at(sb[1], ((1, 9), (11, 4))) == [R.LEAVES] * 2 and at(sb[1], ((3, 15), (3, 14), (2, 15), (2, 14))) == [R.INVALID] * 4
    assert at(sb[1], ((14, 9),)) == [R.TRACKED] and db[1, :, 14, 9].tolist() == [0.0, -14.0]
    free = R.walk_ref("16x24-special", 0, 2, False)["state"][0, :, 0]
    assert at(free[2], ((8, 8), (9, 2), (10, 9))) == [R.TRACKED] * 3                  # nothing reads the checking field


def test_huge_entries_of_the_checking_array_are_read_by_living_tracks():
    """the special clip's 1e30 at chain_ref.HUGE_AT: the owner leaves by the stepping array, its three neighbours stay tracked through
    that step and have the entry as a corner of weight 0 in BOTH arrays.  That the checking array's entry is read there: a NaN in its
    place, in the checking array alone, turns exactly those neighbours `unmatched` at that step.  Both precisions, both directions."""
    fwd, bwd = R.make_case("16x24-special")
    for dtype in (torch.float64, torch.float32):
        for j, c, y, x, v in R.HUGE_AT:
            assert float(fwd[0, j, c, y, x]) == float(bwd[0, j, c, y, x]) == float(torch.tensor(v, dtype=torch.float32))
            near = [(y, x - 1), (y - 1, x), (y - 1, x - 1)]
            for start, stop, slot, checking in ((0, 2, j + 1, "bwd"), (2, 0, 2 - j, "fwd")):
                base = R.chain_ref(fwd, bwd, start, stop, True, dtype=dtype)
                s = base["state"][0, :, 0]
                assert int(s[slot, y, x]) == R.LEAVES and int(s[slot - 1, y, x]) == R.TRACKED
                assert [int(s[slot, yy, xx]) for yy, xx in near] == [R.TRACKED] * 3
                assert all(base["disp"][0, slot, :, yy, xx].tolist() == [0.0, 0.0] for yy, xx in near)      # 0 * 1e30 = 0
                f2, b2 = fwd.clone(), bwd.clone()
                (b2 if checking == "bwd" else f2)[0, j, c, y, x] = float("nan")
                s2 = R.chain_ref(f2, b2, start, stop, True, dtype=dtype)["state"][0, :, 0]
                changed = (s2[slot] != s[slot]).nonzero().tolist()
                assert sorted(changed) == sorted([list(p) for p in near]), (dtype, j, start, changed)
                assert [int(s2[slot, yy, xx]) for yy, xx in near] == [R.UNMATCHED] * 3


def test_huge_checking_value_with_weight_one_overflows_as_the_header_says():
    """chain_ref.huge_clip: a living track reads g = 1e30 with weight 1.  The fp32 run, which is what the kernel is compared with here:
    e2 = m = inf, so with a1 = 0.01 bound = inf, inf <= inf holds and the track is tracked with D = 0; with a1 = 0 bound is NaN and it
    is inconsistent.  The float64 run cannot follow (1e60 > 1e58: inconsistent either way), which is why this clip is not among
    CASES.  Zeroing the entry changes the a1 = 0 result: it is read."""
    fwd, bwd = R.huge_clip()
    for start, stop, (y, x), arr in ((0, 1, (6, 7), bwd), (1, 0, (9, 12), fwd)):
        for a1, want in ((0.01, R.TRACKED), (0.0, R.INCONSISTENT)):
            r32 = R.chain_ref(fwd, bwd, start, stop, True, a1, 0.5, torch.float32)
            assert int(r32["state"][0, 1, 0, y, x]) == want and int(r32["life"][0, 0, y, x]) == (1 if want == R.TRACKED else 0)
            assert torch.isinf(r32["margin"][0, 0, 0, y, x]) or torch.isnan(r32["margin"][0, 0, 0, y, x])
            if want == R.TRACKED:
                assert r32["disp"][0, 1, :, y, x].tolist() == [0.0, 0.0]
            others = torch.ones(16, 24, dtype=torch.bool)
            others[y, x] = False
            oy, ox = (9, 12) if (y, x) == (6, 7) else (6, 7)              # the other entry is this walk's stepping field: it leaves
            others[oy, ox] = False
            assert int(r32["state"][0, 1, 0, oy, ox]) == R.LEAVES and bool((r32["state"][0, 1, 0][others] == R.TRACKED).all())
            assert int(R.chain_ref(fwd, bwd, start, stop, True, a1, 0.5, torch.float64)["state"][0, 1, 0, y, x]) == R.INCONSISTENT
        zeroed = arr.clone()
        zeroed[0, 0, :, y, x] = 0.0
        pair = (fwd, zeroed) if arr is bwd else (zeroed, bwd)
        assert int(R.chain_ref(*pair, start, stop, True, 0.0, 0.5, torch.float32)["state"][0, 1, 0, y, x]) == R.TRACKED


def test_composite_restatement():
    """the rectangle scene: a layer painted on the rectangle in frame 0 lands with alpha 1 exactly on its place in every frame"""
    H, W, T, rect = 19, 70, 3, R.RECT_19x70
    fwd, bwd = R.rect_clip(H, W, [rect], T)
    disp = torch.stack([R.chain_ref(fwd, bwd, t, 0, True)["disp"][:, -1] for t in range(T + 1)], 1)
    gen = torch.Generator().manual_seed(3)
    clip = torch.randn(1, T + 1, 3, H, W, generator=gen)
    layer, paint = torch.zeros(1, 4, H, W), torch.tensor([0.25, -0.5, 0.75, 1.0])
    layer[0, :, R.rect_mask(H, W, rect, 0)] = paint[:, None]
    out = R.composite_ref(clip, layer, disp)
    for t in range(T + 1):
        on = R.rect_mask(H, W, rect, t)
        assert 0 < int(on.sum()) and torch.equal(out[0, t][:, on], paint[:3, None].double().expand(-1, int(on.sum())))
        assert torch.equal(out[0, t][:, ~on], clip[0, t][:, ~on].double())


# ------------------------------------------------------------------------------------------------------------------- argument errors
def test_argument_errors_without_gpu(lib):
    buf = (ctypes.c_float * 1024)()
    base = ctypes.addressof(buf)
    base += -base % 16
    p = ctypes.c_void_p(base)
    ok = lambda rc, word: rc == -1 and word in lib.ofd_last_error()

    def chain(ptrs=None, shape=(1, 2, 4, 4), start=0, stop=2, use_check=1, a1=0.01, a2=0.5, all_steps=1):
        ptrs = ptrs if ptrs is not None else [p] * 5
        return lib.ofd_flow_chain(*ptrs, *shape, start, stop, use_check, a1, a2, all_steps, None)

    def chain_to(ptrs=None, shape=(1, 2, 4, 4), anchor=0, t0=0, nt=3, use_check=1, a1=0.01, a2=0.5):
        ptrs = ptrs if ptrs is not None else [p] * 4
        return lib.ofd_flow_chain_to(*ptrs, *shape, anchor, t0, nt, use_check, a1, a2, None)

    def composite(ptrs=None, shape=(1, 3, 3, 4, 4)):
        ptrs = ptrs if ptrs is not None else [p] * 4
        return lib.ofd_layer_composite(*ptrs, *shape, None)
    for k in (2, 3, 4):                                                     # the outputs are required
        assert ok(chain([None if j == k else p for j in range(5)]), b"null"), k
    assert ok(chain([None, p, p, p, p]), b"null") and ok(chain([p, None, p, p, p]), b"null")          # ahead: steps by fwd, checks by bwd
    assert ok(chain([p, None, p, p, p], start=2, stop=0, use_check=0), b"null")                       # back: steps by bwd
    assert ok(chain([None, p, p, p, p], start=2, stop=0), b"null")                                    # ... and checks by fwd
    for k in range(4):
        assert ok(chain_to([None if j == k else p for j in range(4)]), b"null"), k
        assert ok(composite([None if j == k else p for j in range(4)]), b"null"), k
    for shape in ((0, 2, 4, 4), (1, 2, 0, 4), (1, 2, 4, -1), (1, 2, 32769, 4), (1, 2, 4, 32769), (1 << 14, 2, 1 << 15, 1 << 15)):
        assert ok(chain(shape=shape), b"shape") and ok(chain_to(shape=shape), b"shape"), shape
    for shape in ((1, 0, 4, 4), (1, -1, 4, 4), (1, 4097, 4, 4)):
        assert ok(chain(shape=shape, stop=0), b"T=") and ok(chain_to(shape=shape, nt=1), b"T="), shape
    assert ok(chain_to(shape=(1 << 10, 4096, 1 << 13, 1 << 13), nt=4097), b"shape")                   # nt * B * tiles >= 2^30
    for start, stop in ((-1, 2), (3, 2), (0, 3), (0, -1)):
        assert ok(chain(start=start, stop=stop), b"frames"), (start, stop)
    for anchor, t0, nt in ((-1, 0, 3), (3, 0, 3), (0, -1, 1), (0, 0, 0), (0, 0, 4), (0, 3, 1), (0, 2, 2)):
        assert ok(chain_to(anchor=anchor, t0=t0, nt=nt), b"frames"), (anchor, t0, nt)
    for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
        assert ok(chain(a1=bad), b"finite") and ok(chain(a2=bad), b"finite") and ok(chain_to(a1=bad), b"finite") and ok(chain_to(a2=bad), b"finite")
    assert ok(chain(use_check=2), b"use_check") and ok(chain(all_steps=-1), b"all_steps") and ok(chain_to(use_check=-1), b"use_check")
    for shape in ((0, 3, 3, 4, 4), (1, 3, 3, 0, 4), (1, 3, 3, 4, 32769), (1 << 14, 3, 3, 1 << 15, 1 << 15)):
        assert ok(composite(shape=shape), b"shape"), shape
    for C in (0, 9, -1):
        assert ok(composite(shape=(1, 3, C, 4, 4)), b"C="), C
    for n in (0, -1, 4098):
        assert ok(composite(shape=(1, n, 3, 4, 4)), b"n="), n
    # outputs that share a byte with an input array, in otherwise valid calls: rejected before the launch.  (1, 2, 4, 4): fwd and bwd
    # hold 64 floats, disp 96, state 48 bytes, life 16 ints; the pointers below are 512 bytes apart unless they are made to meet
    q = [ctypes.c_void_p(base + 512 * k) for k in range(5)]
    at = lambda k, off: ctypes.c_void_p(base + 512 * k + off)
    for ptrs in ([q[0], q[1], q[0], q[3], q[4]], [q[0], q[1], q[2], q[1], q[4]], [q[0], q[1], q[2], q[3], at(0, 252)],
                 [q[0], q[1], at(1, 4), q[3], q[4]], [q[0], at(2, 380), q[2], q[3], q[4]]):
        assert ok(chain(ptrs), b"alias"), [p_.value - base for p_ in ptrs]
    assert ok(chain([q[0], None, q[0], q[3], q[4]], use_check=0), b"alias")                          # a missing array aliases nothing
    for ptrs in ([q[0], q[1], q[1], q[3]], [q[0], q[1], q[2], at(0, 255)]):
        assert ok(chain_to(ptrs), b"alias"), [p_.value - base for p_ in ptrs]
    # composite (1, 3, 3, 4, 4): frames and out 144 floats (576 bytes), layer 64, disp 96; 1024 bytes apart
    big = (ctypes.c_float * 2048)()
    b0 = ctypes.addressof(big)
    r = [ctypes.c_void_p(b0 + 1024 * k) for k in range(4)]
    for ptrs in ([r[0], r[1], r[2], r[0]], [r[0], r[1], r[2], r[1]], [r[0], r[1], r[2], ctypes.c_void_p(b0 + 2048 + 380)],
                 [r[0], r[1], r[2], ctypes.c_void_p(b0 + 572)]):
        assert ok(composite(ptrs), b"alias"), [p_.value - b0 for p_ in ptrs]


def test_signatures_and_version(lib):
    from opticalflowdiffusion_amd import _lib
    assert {"ofd_flow_chain", "ofd_flow_chain_to", "ofd_layer_composite"} <= set(_lib.SIGNATURES)
    assert lib.ofd_version() >= 12                                          # the minor went up with the new symbols


# ------------------------------------------------------------------------------------------------------------------------ host rules
def test_warp_functions_argument_errors(lib):
    import opticalflowdiffusion_amd as pkg
    from opticalflowdiffusion_amd import _lib
    from opticalflowdiffusion_amd.warp import FlowChain, chain_flows, chain_flows_to, composite_layer
    assert pkg.chain_flows is chain_flows and pkg.chain_flows_to is chain_flows_to and pkg.composite_layer is composite_layer
    assert pkg.FlowChain is FlowChain and FlowChain._fields == ("disp", "state", "life")
    assert (pkg.STATE_HELD, pkg.STATE_INCONSISTENT, pkg.STATE_LEAVES_FRAME, pkg.STATE_UNMATCHED, pkg.STATE_INVALID) == (
        R.TRACKED, R.INCONSISTENT, R.LEAVES, R.UNMATCHED, R.INVALID)
    fl = torch.zeros(1, 2, 2, 8, 8)
    for bad in (dict(fwd=torch.zeros(2, 2, 8, 8)), dict(fwd=torch.zeros(1, 2, 3, 8, 8)), dict(fwd=None), dict(bwd=torch.zeros(1, 2, 2, 8, 9)),
                dict(bwd=torch.zeros(1, 3, 2, 8, 8)), dict(fwd=torch.zeros(0, 2, 2, 8, 8), bwd=torch.zeros(0, 2, 2, 8, 8)),
                dict(fwd=fl.int(), bwd=fl.int())):
        args = dict(fwd=fl, bwd=fl)
        args.update(bad)
        with pytest.raises(ValueError, match="chain_flows:"):
            chain_flows(**args)
        with pytest.raises(ValueError, match="chain_flows_to:"):
            chain_flows_to(**args)
    with pytest.raises(ValueError, match="bwd is needed"):
        chain_flows_to(fl, None)
    for kw in (dict(start=-1), dict(start=3), dict(stop=3), dict(stop=1.0), dict(start=True), dict(check=1), dict(all_steps=1),
               dict(a1=-0.1), dict(a2=float("nan")), dict(a1="x")):
        with pytest.raises(ValueError, match="chain_flows"):
            chain_flows(fl, fl, **kw)
    with pytest.raises(ValueError, match="steps by bwd"):
        chain_flows(fl, None, start=2, stop=0)
    with pytest.raises(ValueError, match="check=True needs"):
        chain_flows(fl, None, check=True)
    for kw in (dict(anchor=-1), dict(anchor=3), dict(anchor=0.0), dict(check=None), dict(a1=float("inf")), dict(a2=-1)):
        with pytest.raises(ValueError, match="chain_flows_to"):
            chain_flows_to(fl, fl, **kw)
    clip, layer, disp = torch.zeros(1, 3, 3, 8, 8), torch.zeros(1, 4, 8, 8), torch.zeros(1, 3, 2, 8, 8)
    for bad in (dict(frames=torch.zeros(1, 3, 8, 8)), dict(frames=torch.zeros(1, 3, 9, 8, 8)), dict(frames=None), dict(layer=torch.zeros(1, 3, 8, 8)),
                dict(layer=None), dict(disp=torch.zeros(1, 2, 2, 8, 8)), dict(disp=torch.zeros(1, 3, 2, 8, 9)), dict(disp=disp.long()),
                dict(premultiplied=1)):
        args = dict(frames=clip, layer=layer, disp=disp)
        args.update(bad)
        with pytest.raises(ValueError, match="composite_layer"):
            composite_layer(**args)
    for call in (lambda: chain_flows(fl.clone().requires_grad_(True), fl), lambda: chain_flows_to(fl, fl.clone().requires_grad_(True)),
                 lambda: composite_layer(clip, layer.clone().requires_grad_(True), disp)):
        with pytest.raises(_lib.OfdError, match="forward only"):
            call()
    for call in (lambda: chain_flows(fl, fl), lambda: chain_flows(fl), lambda: chain_flows_to(fl, fl), lambda: composite_layer(clip, layer, disp)):
        with pytest.raises(_lib.OfdError, match="GPU only"):                # there is no CPU path
            call()


def test_flow_diffuser_clip_host_logic(host_registry, monkeypatch):       # noqa: F811
    """the rules of estimate_flow_clip, track and propagate raise before any model or engine call; the pairs go through
    estimate_flow_pair in the order (sample, pair), split by pairs_per_call; given flows reach the warp functions untouched"""
    from opticalflowdiffusion_amd import FlowDiffuser
    from opticalflowdiffusion_amd import flow_diffuser as FDM
    H, W, B, T = 16, 24, 2, 3
    fd = FlowDiffuser(dict(target="flow", image_size=[H, W], timesteps=20, flow_max=20))
    try:
        clip = torch.arange(B * (T + 1) * 3 * H * W, dtype=torch.float32).view(B, T + 1, 3, H, W)
        fl, layer = torch.zeros(B, T, 2, H, W), torch.zeros(B, 4, H, W)

        def no_call(*a, **kw):
            raise AssertionError("a model or engine call before the arguments were checked")
        for attr in ("sample", "estimate_flow", "estimate_flow_pair"):
            monkeypatch.setattr(fd, attr, no_call)
        for attr in ("chain_flows", "chain_flows_to", "composite_layer"):
            monkeypatch.setattr(FDM, attr, no_call)
        for bad in (torch.zeros(B, 3, H, W), torch.zeros(B, 1, 3, H, W), torch.zeros(B, 4, 2, H, W), None):
            for call in (lambda c: fd.estimate_flow_clip(c), lambda c: fd.track(c), lambda c: fd.propagate(c, layer)):
                with pytest.raises(ValueError, match="clip must be"):
                    call(bad)
        for ppc in (0, -1, 1.0, True):
            with pytest.raises(ValueError, match="pairs_per_call"):
                fd.estimate_flow_clip(clip, pairs_per_call=ppc)
        for name, call in (("track", lambda **kw: fd.track(clip, **kw)), ("propagate", lambda **kw: fd.propagate(clip, layer, **kw))):
            with pytest.raises(ValueError, match="come together"):
                call(fwd=fl)
            with pytest.raises(ValueError, match="come together"):
                call(bwd=fl)
            with pytest.raises(ValueError, match="sampling arguments"):
                call(fwd=fl, bwd=fl, guidance_scale=2.0)
            with pytest.raises(ValueError, match="fwd must be"):
                call(fwd=fl[:, :2], bwd=fl)
            with pytest.raises(ValueError, match="bwd must be"):
                call(fwd=fl, bwd=torch.zeros(B, T, 2, H, W + 1))
            for kw in (dict(a1=-1.0), dict(a2=float("nan")), dict(check=None), dict(check=1)):
                with pytest.raises(ValueError, match=name):
                    call(fwd=fl, bwd=fl, **kw)
        for kw in (dict(start=-1), dict(start=T + 1), dict(stop=T + 1), dict(stop=1.5), dict(start=True)):
            with pytest.raises(ValueError, match="track: st"):
                fd.track(clip, fwd=fl, bwd=fl, **kw)
        for kw in (dict(anchor=-1), dict(anchor=T + 1), dict(anchor=0.0), dict(premultiplied=0)):
            with pytest.raises(ValueError, match="propagate"):
                fd.propagate(clip, layer, fwd=fl, bwd=fl, **kw)
        with pytest.raises(ValueError, match="layer must be"):
            fd.propagate(clip, torch.zeros(B, 3, H, W), fwd=fl, bwd=fl)
        from opticalflowdiffusion_amd import _lib
        grad = lambda t: t.clone().requires_grad_(True)
        for call in (lambda: fd.track(grad(clip), fwd=fl, bwd=fl), lambda: fd.track(clip, fwd=grad(fl), bwd=fl), lambda: fd.track(grad(clip)),
                     lambda: fd.propagate(grad(clip), layer, fwd=fl, bwd=fl), lambda: fd.propagate(clip, layer, fwd=fl, bwd=grad(fl)),
                     lambda: fd.propagate(clip, grad(layer), fwd=fl, bwd=fl), lambda: fd.propagate(grad(clip), layer)):
            with pytest.raises(_lib.OfdError, match="forward only"):        # nothing is detached on the quiet
                call()
        monkeypatch.setattr(fd, "latent", True)
        for call in (lambda: fd.estimate_flow_clip(clip), lambda: fd.track(clip, fwd=fl, bwd=fl), lambda: fd.propagate(clip, layer, fwd=fl, bwd=fl)):
            with pytest.raises(ValueError, match="latent"):
                call()
        monkeypatch.setattr(fd, "latent", False)
        monkeypatch.setattr(fd, "is_diffusion", False)
        with pytest.raises(ValueError, match="diffusion model"):
            fd.track(clip)
        monkeypatch.setattr(fd, "is_diffusion", True)
        # the pairs, with the model replaced
        calls = []

        def fake_pair(a, b, **kw):
            calls.append((a, b, kw))
            return a[:, :2] + 0.5, b[:, :2] - 0.5, None
        monkeypatch.setattr(fd, "estimate_flow_pair", fake_pair)
        first, second = clip[:, :-1].reshape(B * T, 3, H, W), clip[:, 1:].reshape(B * T, 3, H, W)
        fwd, bwd = fd.estimate_flow_clip(clip, guidance_scale=2.0, dilate=1)
        assert len(calls) == 1 and calls[0][2] == dict(refine=0, guidance_scale=2.0, dilate=1)
        assert torch.equal(calls[0][0], first) and torch.equal(calls[0][1], second)
        assert torch.equal(fwd, (first[:, :2] + 0.5).view(B, T, 2, H, W)) and torch.equal(bwd, (second[:, :2] - 0.5).view(B, T, 2, H, W))
        del calls[:]
        fwd4, bwd4 = fd.estimate_flow_clip(clip, refine=2, pairs_per_call=4)
        assert [c[0].shape[0] for c in calls] == [4, 2] and all(c[2] == dict(refine=2) for c in calls)
        assert torch.equal(torch.cat([c[0] for c in calls]), first) and torch.equal(fwd4, fwd) and torch.equal(bwd4, bwd)
        # track and propagate hand down what they were given, or what estimate_flow_clip returns
        seen = {}
        chain = object()
        monkeypatch.setattr(FDM, "chain_flows", lambda f, b, **kw: seen.update(chain=(f, b, kw)) or chain)
        monkeypatch.setattr(FDM, "chain_flows_to", lambda f, b, **kw: seen.update(to=(f, b, kw)) or ("disp", "state"))
        monkeypatch.setattr(FDM, "composite_layer", lambda c, l, d, **kw: seen.update(comp=(c, l, d, kw)) or "video")
        monkeypatch.setattr(fd, "estimate_flow_clip", lambda c, **kw: seen.update(est=kw) or (fwd, bwd))
        got = fd.track(clip, start=1, stop=3, fwd=fl, bwd=fl, check=False, a1=0.02, a2=0.25)
        assert got[0] is chain and got[1] is fl and got[2] is fl and "est" not in seen
        assert seen["chain"][0] is fl and seen["chain"][2] == dict(start=1, stop=3, check=False, a1=0.02, a2=0.25)
        got = fd.track(clip, refine=1, pairs_per_call=2, guidance_scale=2.0)
        assert seen["est"] == dict(refine=1, pairs_per_call=2, guidance_scale=2.0) and got[1] is fwd and got[2] is bwd
        assert seen["chain"][0] is fwd and seen["chain"][1] is bwd and seen["chain"][2] == dict(start=0, stop=None, check=True, a1=0.01, a2=0.5)
        del seen["est"]
        got = fd.propagate(clip, layer, anchor=2, fwd=fl, bwd=fl, premultiplied=False)
        assert got[0] == "video" and got[1] is fl and got[2] is fl and "est" not in seen
        assert seen["to"][0] is fl and seen["to"][2] == dict(anchor=2, check=True, a1=0.01, a2=0.5)
        assert seen["comp"][1] is layer and seen["comp"][2] == "disp" and seen["comp"][3] == dict(premultiplied=False)
        assert seen["comp"][0] is clip
        got = fd.propagate(clip, layer, photo_scale=0.5)
        assert seen["est"] == dict(photo_scale=0.5) and got[1] is fwd and seen["to"][0] is fwd
    finally:
        fd.unet._handle = None
