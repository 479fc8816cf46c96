"""The order in which the fixed-order sums add, restated in NumPy float64 on the host and compared with the kernels BIT FOR BIT (no
tolerance).  Run-to-run equality, which the other tests check, survives a reordering of the adds; this test does not.  The order is the
one csrc/reduce.h writes down:
    per thread    the thread's elements in ascending index, float32(d * d) widened to double
    per wave      a 64-lane tree, offsets 32, 16, ..., 1: lane i takes lane i + offset
    per workgroup the four wave results as (0 + 1) + (2 + 3)
    the total     thread t adds partials t, t + 256, ... in ascending order, then a 256-slot tree, k = 128, ..., 1: slot i takes slot i + k
and, for the per-sample sums, nan_mse_rows_total_kernel's own: lane l of a wave adds the partials l, l + 64, ... of one sample, the 64-lane
tree joins them, and one thread adds the samples in ascending order."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BLOCKS = 2048          # NAN_MSE_BLOCKS, ROWS_BLOCKS


def _strided(x, stride):
    """x (..., n) -> (..., stride): column c is x[c] + x[c + stride] + ... added in ascending order from +0.0"""
    n = x.shape[-1]
    k = -(-n // stride)
    pad = np.zeros(x.shape[:-1] + (k * stride,), dtype=np.float64)
    pad[..., :n] = x
    pad = pad.reshape(x.shape[:-1] + (k, stride))
    acc = np.zeros(x.shape[:-1] + (stride,), dtype=np.float64)
    for i in range(k):
        acc = acc + pad[..., i, :]
    return acc


def _tree(x):
    """x (..., 2^m) -> (...): step k = 2^(m-1), ..., 1 replaces slot i < k by slot i + slot (i + k); the result is slot 0"""
    x = x.copy()
    k = x.shape[-1] // 2
    while k > 0:
        x[..., :k] = x[..., :k] + x[..., k:2 * k]
        k //= 2
    return x[..., 0]


def _workgroup(x):
    """x (..., 256) per-thread values -> (...): the 64-lane tree of each wave, then (w0 + w1) + (w2 + w3)"""
    w = _tree(x.reshape(x.shape[:-1] + (4, 64)))
    return (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])


def _total(part):
    """part (n,) -> scalar: the ascending per-thread pre-sum, then the 256-slot tree"""
    return _tree(_strided(part, 256))


def _inputs(shape, seed):
    """standard normal pairs; about 3 % of pred is NaN and another 3 % of target"""
    g = np.random.default_rng(seed)
    p, t = g.standard_normal(shape, dtype=np.float32), g.standard_normal(shape, dtype=np.float32)
    p[g.random(shape) < 0.03] = np.nan
    t[g.random(shape) < 0.03] = np.nan
    return p, t


def _squares(p, t):
    """(float32(d * d) as double with +0.0 at the NaN pairs, 1.0 / 0.0 for counted / not)"""
    ok = ~(np.isnan(p) | np.isnan(t))
    d = np.where(ok, p - t, np.float32(0.0)).astype(np.float32)
    return (d * d).astype(np.float64), ok.astype(np.float64)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("n", [1, 256 * 3 + 17, 2048 * 256 * 2 + 1000])
def test_nan_mse_sum_adds_in_the_stated_order(n):
    from opticalflowdiffusion_amd import _lib as L
    p, t = _inputs((n,), seed=n % 1000)
    want = []
    blocks = min(-(-n // 256), BLOCKS)
    for v in _squares(p, t):
        per_thread = _strided(v, blocks * 256).reshape(blocks, 256)       # thread g = block * 256 + tid takes g, g + blocks * 256, ...
        want.append(_total(_workgroup(per_thread)))
    dp, dt = torch.from_numpy(p).cuda(), torch.from_numpy(t).cuda()
    res = torch.full((L.lib().ofd_nan_mse_result_doubles(),), float("nan"), dtype=torch.float64, device="cuda")
    L.check(L.lib().ofd_nan_mse_sum(L.ptr(dp), L.ptr(dt), n, L.ptr(res), L.stream()))
    got = res[:2].cpu().numpy()
    print("nan_mse_sum", n, got, want)
    assert np.array_equal(_bits(got), _bits(want)), (n, got.tolist(), [float(w) for w in want])


# the last two are not in the issue's list: a workgroup that takes more than 256 groups of a sample, so that the two-in-flight loop
# runs as well as its tail, once with one workgroup per sample walking several slots and once with two workgroups per sample
@pytest.mark.parametrize("B,n", [(5, 7 * 9 * 3), (3, 4 * 256 * 6 + 4), (2100, 64), (2100, 1200), (700, 6000)])
def test_nan_mse_rows_adds_in_the_stated_order(B, n):
    from opticalflowdiffusion_amd import _lib as L
    p, t = _inputs((B, n), seed=B)
    vec = 4 if n % 4 == 0 else 1                 # torch's allocations are 16-byte aligned
    units = n // vec
    wps = max(1, min(BLOCKS // B, -(-units // 256)))
    pairs = []
    for v in _squares(p, t):
        # thread tid of slot (b, w) takes the groups w * 256 + tid, stepping wps * 256, and the vec elements of a group in order:
        # element e of the sample belongs to column (e // vec) % (wps * 256), and a column's elements are added in ascending e
        step = wps * 256
        k = -(-units // step)
        pad = np.zeros((B, k * step * vec), dtype=np.float64)
        pad[:, :n] = v
        pad = pad.reshape(B, k, step, vec)
        acc = np.zeros((B, step), dtype=np.float64)
        for i in range(k):
            for j in range(vec):
                acc = acc + pad[:, i, :, j]
        part = _workgroup(acc.reshape(B, wps, 256))                        # (B, wps)
        pairs.append(part[:, 0] if wps == 1 else _tree(_strided(part, 64)))
    S, N = pairs
    want = np.empty(2 + 2 * B, dtype=np.float64)
    want[0], want[1] = np.add.accumulate(S)[-1], np.add.accumulate(N)[-1]   # one thread, ascending b (weight NULL: 1.0 * S_b)
    want[2::2], want[3::2] = S, N
    dp, dt = torch.from_numpy(p).cuda(), torch.from_numpy(t).cuda()
    assert dp.data_ptr() % 16 == 0 and dt.data_ptr() % 16 == 0
    res = torch.full((L.lib().ofd_nan_mse_rows_result_doubles(B),), float("nan"), dtype=torch.float64, device="cuda")
    L.check(L.lib().ofd_nan_mse_rows(L.ptr(dp), L.ptr(dt), None, B, n, L.ptr(res), L.stream()))
    got = res[:2 + 2 * B].cpu().numpy()
    print("nan_mse_rows", B, n, "wps", wps, got[:4], want[:4])
    bad = np.flatnonzero(_bits(got) != _bits(want))
    assert bad.size == 0, (B, n, wps, bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())
