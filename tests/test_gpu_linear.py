"""GPU (MI355X): the split-f16 linear engine (ehm_linear_split, csrc/linear.hip) and the small kernels beside it, each against a
float64 reference of the same operation computed on the device from the exact float32 inputs.

The linear engine computes

    Y = relu_out( [relu_in0(A0) | A1] . W^T + bias + group_bias[row // rows_per_group] )
    colmax[g] = max(prefill, max of Y over the valid rows of group g)

on X2 operands (csrc/gcn_dev.h: 32 hi halves + 32 lo halves per 32-k group).  Y is read back with ehm_gcn_unpack_activations(..., 32).

Error model (every bound of the engine below is derived from it; A' is the operand after relu_in0 / the lift, W unscaled, s = w_scale):
  * an operand x is stored as hi + lo, hi = f16(x), lo = f16(x - hi): |x - hi - lo| <= 2^-22 |x| + 2^-25 (the last term: lo below
    the f16 normal range).  The hi-only tier keeps hi alone: |x - hi| <= 2^-11 |x| + 2^-25.
  * a product is ah.wh + ah.wl + al.wh, exact in f32; the dropped al.wl and the two representation errors are at most 3 . 2^-22 |a||w|
    per product (hi-only: 2 . 2^-11 |a||w|), plus 2^-25 (|w| + |a| / s) from the floor above.
  * W is random-signed and drawn independently of A in every case here, so the K per-product errors add like a random walk: their
    scale is R = sqrt((A'^2) . (W^2)^T), not the worst case S = |A'| . |W|^T + |bias| + |gbias|, which is loose by about sqrt(K) for
    such operands and would let an engine that drops a whole correction product pass.  The bounds take 8 R (split) and 4 R (hi-only)
    for the tail of that walk over up to 10^6 outputs.
  * f32 accumulation: at most 3K roundings (K hi-only), each <= 2^-24 of a partial sum, whose scale is R + |A'.W^T|: again a random
    walk, 4 sqrt(3K) . 2^-24 (R + |A'.W^T|).
  * epilogue: one f32 rounding of the fma with the biases and the re-split of Y: 2^-21 |Y| + 2^-25 (hi-only: 2^-10 |Y| + 2^-24).
So
    split:    tol = 8 . 2^-20 R + 2^-22 sqrt(3K) (R + |A'.W^T|) + 2^-25 (sum|w| + sum|a| / s) + 2^-21 |Y| + 2^-25
    hi-only:  tol = 4 . 2^-10 R + 2^-22 sqrt(K)  (R + |A'.W^T|) + 2^-25 (sum|w| + sum|a| / s) + 2^-10 |Y| + 2^-24
and colmax is within the largest tol of its group's valid rows (max is 1-Lipschitz).  An engine without one correction product
(al.wh) is off by about 2^-12.3 R per output: on the MI355X such an engine failed every split-tier case below, the descriptor matrix by
14 to 85 times its bound, while the engine itself stays under a tenth of it.  Every test prints its largest error / bound ratio."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

LBM, LBN = 192, 128                 # output tile of csrc/linear.hip
PAD = 6.0                           # rows past valid_rows_per_group: large, so that any leak into colmax shows
SENTINEL = 0x5A5A                   # bit pattern the hi-only tier must leave in the lo halves of Y


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def L():
    from egohmr_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def cus(dev):
    return torch.cuda.get_device_properties(0).multi_processor_count


def _check(rc, L):
    assert rc == 0, (rc, L.ehm_last_error())


def _x2(L, X, scale=1.0):
    """float32 [rows, K] (device) -> X2 [rows, K] (ehm_split_pack)"""
    rows, K = X.shape
    out = torch.empty(rows, K, device=X.device)
    _check(L.ehm_split_pack(X.data_ptr(), out.data_ptr(), rows, K, K, float(scale), None), L)
    return out


def _unx2(L, Y, rows=None, row0=0):
    """X2 [*, N] -> float32 [rows, N] (ehm_gcn_unpack_activations, group 32), from row row0 on"""
    N = Y.shape[1]
    rows = Y.shape[0] - row0 if rows is None else rows
    out = torch.empty(rows, N, device=Y.device)
    _check(L.ehm_gcn_unpack_activations(Y.data_ptr() + row0 * N * 4, out.data_ptr(), rows, N, 32, None), L)
    return out


def _halves(Y):
    """X2 [rows, N] -> (hi, lo) as int16 [rows, N] bit patterns"""
    rows, N = Y.shape
    h = Y.view(torch.int16).view(rows, N // 32, 2, 32)
    return h[:, :, 0, :].reshape(rows, N), h[:, :, 1, :].reshape(rows, N)


def _schedule(cus, M, N):
    """ehm_linear_split's grid and tile order: (G, xcd_order), exactly as the library computes them"""
    tiles = (M // LBM) * (N // LBN)
    G = min(2 * cus, tiles)
    return G, (G % 8 == 0) and ((G // 8) % (N // LBN) == 0)


def _tiles_of(b, G, xcd, m_tiles, n_tiles):
    """tile_of (csrc/linear.hip) for block b: its (m, n) tiles in iteration order"""
    out, it = [], 0
    while True:
        if xcd:
            x, j, per = b & 7, b >> 3, (G >> 3) // n_tiles
            m, n = (it * per + j // n_tiles) * 8 + x, j % n_tiles
        else:
            t = it * G + b
            m, n = t // n_tiles, t % n_tiles
        if m >= m_tiles:
            return out
        out.append((m, n))
        it += 1


def _tol(Ap, Aabs, W, K, w_scale, hi_only, y):
    """The error model of the module docstring: (A'.W^T, tol) for operand rows Ap [rows, K] (float64), Aabs >= |Ap| (the lift's generated
    operand: its magnitude before rounding), W [N, K] float32, y = the reference output [rows, N]"""
    Wd = W.double()
    P = Ap @ Wd.t()
    R = torch.sqrt((Aabs * Aabs) @ (Wd * Wd).t())
    floor = 2.0 ** -25 * (Wd.abs().sum(1)[None, :] + Aabs.sum(1, keepdim=True) / w_scale)
    if hi_only:
        return P, 4 * 2.0 ** -10 * R + 2.0 ** -22 * math.sqrt(K) * (R + P.abs()) + floor + 2.0 ** -10 * y.abs() + 2.0 ** -24
    return P, 8 * 2.0 ** -20 * R + 2.0 ** -22 * math.sqrt(3 * K) * (R + P.abs()) + floor + 2.0 ** -21 * y.abs() + 2.0 ** -25


class Case:
    """One ehm_linear_split launch: seeded float32 inputs on the device, their X2 forms, the descriptor, and the float64 reference.
    mode: plain | relu_in0 | dual | lift;  bias: none | bias | dense (group bias, stride 0) | strided (bias + a group-bias matrix read
    from column N with a row stride of 2N + 32, the PointNet's (vs, H) form)."""

    def __init__(self, L, dev, *, M, N, K0, K1=0, rpg=None, valid=0, mode="plain", bias="none", relu_out=0, seed=0, w_scale=1024.0,
                 hi_only=False, pad=PAD):
        assert (K1 > 0) == (mode == "dual")
        self.L, self.dev = L, dev
        self.M, self.N, self.K0, self.K1, self.K = M, N, K0, K1, K0 + K1
        self.rpg = rpg or M
        self.groups, self.valid = M // self.rpg, valid
        self.nv = valid or self.rpg
        self.mode, self.bias_kind, self.relu_out, self.w_scale, self.hi_only = mode, bias, relu_out, w_scale, hi_only
        g = torch.Generator(device=dev).manual_seed(seed)
        rnd = lambda *s: torch.randn(*s, generator=g, device=dev)
        self.W = rnd(N, self.K) / math.sqrt(self.K)
        self.A0 = self.A1 = self.pts = None
        if mode == "lift":
            self.pts = torch.rand(self.groups, self.nv, 3, generator=g, device=dev) * 2 - 1
            self.Wpos, self.bpos = rnd(K0, 3) * 0.7, rnd(K0) * 0.3
            self.W4 = torch.cat([self.Wpos, self.bpos[:, None]], 1).contiguous()
        else:
            self.A0 = rnd(M, K0)
            self.A1 = rnd(M, K1) if K1 else None
            for A in (self.A0, self.A1):
                if A is not None and self.nv < self.rpg:
                    A.view(self.groups, self.rpg, -1)[:, self.nv:] = pad
        self.bias = rnd(N) if bias in ("bias", "strided") else None
        self.gb_full, self.gb_off, self.gb_stride = None, 0, 0
        if bias == "dense":
            self.gb_full = rnd(self.groups, N)
        elif bias == "strided":
            self.gb_full, self.gb_off, self.gb_stride = rnd(self.groups, 2 * N + 32), N, 2 * N + 32
        self.Wx2 = _x2(L, self.W, w_scale)
        self.A0x2 = _x2(L, self.A0) if self.A0 is not None else None
        self.A1x2 = _x2(L, self.A1) if self.A1 is not None else None

    def desc(self, Y, colmax):
        from egohmr_amd import _lib
        lift = self.mode == "lift"
        return _lib.LinearDesc(
            A0=None if lift else self.A0x2.data_ptr(), A1=self.A1x2.data_ptr() if self.K1 else None, W=self.Wx2.data_ptr(),
            bias=self.bias.data_ptr() if self.bias is not None else None,
            group_bias=self.gb_full.data_ptr() + 4 * self.gb_off if self.gb_full is not None else None,
            Y=Y.data_ptr() if Y is not None else None, colmax=colmax.data_ptr() if colmax is not None else None,
            M=self.M, N=self.N, K0=self.K0, K1=self.K1, rows_per_group=self.rpg, valid_rows_per_group=self.valid,
            relu_in0=int(self.mode == "relu_in0"), relu_out=self.relu_out, w_scale=self.w_scale,
            lift_points=self.pts.data_ptr() if lift else None, lift_W4=self.W4.data_ptr() if lift else None,
            hi_only=int(self.hi_only), group_bias_stride=self.gb_stride)

    def run(self, y=True, colmax=True, prefill=None, y_fill=None):
        """launch once; returns (Y X2 buffer or None, colmax or None)"""
        Y = None
        if y:
            Y = torch.empty(self.M, self.N, device=self.dev)
            if y_fill is None:
                Y.fill_(float("nan"))
            else:
                Y.view(torch.int16).fill_(y_fill)
        cm = None
        if colmax:
            cm = torch.full((self.groups, self.N), float("-inf"), device=self.dev) if prefill is None else prefill.clone()
        _check(self.L.ehm_linear_split(self.desc(Y, cm), None), self.L)
        torch.cuda.synchronize()
        return Y, cm

    def operand(self, rows):
        """(A', |A'| bound) in float64 for the given row indices (device LongTensor)"""
        if self.mode == "lift":
            grp, i = rows // self.rpg, rows % self.rpg
            p = torch.zeros(rows.numel(), 3, dtype=torch.float64, device=self.dev)
            ok = i < self.nv
            p[ok] = self.pts[grp[ok], i[ok]].double()
            Ap = torch.relu(p @ self.Wpos.double().t() + self.bpos.double())
            return Ap, p.abs() @ self.Wpos.double().abs().t() + self.bpos.double().abs()
        Ap = self.A0[rows].double()
        if self.mode == "relu_in0":
            Ap = torch.relu(Ap)
        if self.A1 is not None:
            Ap = torch.cat([Ap, self.A1[rows].double()], 1)
        return Ap, Ap.abs()

    def reference(self, rows):
        """(Y_ref, tol) [len(rows), N] in float64 for the given rows"""
        Ap, Aabs = self.operand(rows)
        add = torch.zeros(rows.numel(), self.N, dtype=torch.float64, device=self.dev)
        if self.bias is not None:
            add += self.bias.double()[None]
        if self.gb_full is not None:
            add += self.gb_full.double()[rows // self.rpg, self.gb_off:self.gb_off + self.N]
        P = Ap @ self.W.double().t()
        y = P + add
        if self.relu_out:
            y = torch.relu(y)
        return y, _tol(Ap, Aabs, self.W, self.K, self.w_scale, self.hi_only, y)[1]

    def colmax_reference(self, groups=None, chunk_rows=1 << 16):
        """(colmax_ref, tol) [groups, N]: max of Y_ref over the valid rows of each group, and the largest tol among them"""
        groups = range(self.groups) if groups is None else groups
        ref = torch.empty(len(groups), self.N, dtype=torch.float64, device=self.dev)
        tol = torch.empty_like(ref)
        for gi, grp in enumerate(groups):
            mx = torch.full((self.N,), -math.inf, dtype=torch.float64, device=self.dev)
            tl = torch.zeros(self.N, dtype=torch.float64, device=self.dev)
            for r0 in range(0, self.nv, chunk_rows):
                rows = grp * self.rpg + torch.arange(r0, min(r0 + chunk_rows, self.nv), device=self.dev)
                y, t = self.reference(rows)
                mx = torch.maximum(mx, y.max(0).values)
                tl = torch.maximum(tl, t.max(0).values)
            ref[gi], tol[gi] = mx, tl
        return ref, tol


def _ratio(err, tol):
    return float((err / tol).max())


def _check_y(c, Y, rows=None, tag=""):
    """Y (X2, all rows or the given rows) against the reference; returns the largest error / bound ratio"""
    rows = torch.arange(c.M, device=c.dev) if rows is None else rows
    got = _unx2(c.L, Y)[rows].double()
    ref, tol = c.reference(rows)
    assert torch.isfinite(got).all(), tag
    r = _ratio((got - ref).abs(), tol)
    assert r <= 1.0, f"{tag}: Y off by {r:.2f} x the bound (max|err| = {float((got - ref).abs().max()):.3e})"
    return r


def _check_colmax(c, cm, prefill=None, tag=""):
    ref, tol = c.colmax_reference()
    if prefill is not None:
        ref = torch.maximum(ref, prefill.double())
    got = cm.double()
    assert torch.isfinite(got).all(), tag
    r = _ratio((got - ref).abs(), tol)
    assert r <= 1.0, f"{tag}: colmax off by {r:.2f} x the bound (max|err| = {float((got - ref).abs().max()):.3e})"
    return r


# --------------------------------------------------------------------------------------------- descriptor matrix
MODES = ("plain", "relu_in0", "dual", "lift")
BIASES = ("none", "bias", "dense", "strided")
OUTPUTS = (("Y", "colmax"), ("Y",), ("colmax",))
# K per (mode, bias index): the minimum K0 + K1 = 64 (also as 32 + 32), odd K-tile counts (96 = 3, 288 = 9), the PointNet's H + 32 = 288
# and 2H = 512
KS = {"plain": [(64, 0), (96, 0), (288, 0), (512, 0)], "relu_in0": [(64, 0), (288, 0), (96, 0), (256, 0)],
      "dual": [(32, 32), (256, 32), (32, 64), (256, 256)], "lift": [(512, 0), (64, 0), (96, 0), (256, 0)]}
MATRIX = [(MODES[i], BIASES[j], (i + j) % 2, OUTPUTS[(i + 2 * j) % 3], KS[MODES[i]][j]) for i in range(4) for j in range(4)]


def test_descriptor_matrix_is_a_pairwise_cover():
    import itertools
    levels = [MODES, BIASES, (0, 1), OUTPUTS]
    for a, b in itertools.combinations(range(4), 2):
        assert {(r[a], r[b]) for r in MATRIX} == set(itertools.product(levels[a], levels[b])), (a, b)


@pytest.mark.parametrize("mode,bias,relu_out,outs,k", MATRIX, ids=[f"{m}-{b}-relu{r}-{'+'.join(o)}-K{k[0]}+{k[1]}" for m, b, r, o, k in MATRIX])
def test_linear_split_descriptor_matrix_vs_fp64(L, dev, mode, bias, relu_out, outs, k):
    """Split tier, every operand mode x bias form x relu_out x output set (pairwise), three groups of 384 rows with 300 valid: the second
    row tile of a group has 108 valid rows, so its second wave recomputes the maximum over 12."""
    c = Case(L, dev, M=3 * 384, N=256, K0=k[0], K1=k[1], rpg=384, valid=300, mode=mode, bias=bias, relu_out=relu_out,
             seed=100 + 4 * MODES.index(mode) + BIASES.index(bias))
    Y, cm = c.run(y="Y" in outs, colmax="colmax" in outs)
    tag = f"[matrix {mode} {bias} relu_out={relu_out} {outs} K={k}]"
    rs = []
    if Y is not None:
        rs.append(_check_y(c, Y, tag=tag))
    if cm is not None:
        rs.append(_check_colmax(c, cm, tag=tag))
    print(f"{tag} max err/bound = {max(rs):.3f}")


@pytest.mark.parametrize("mode,k", [("plain", (64, 0)), ("relu_in0", (288, 0)), ("dual", (256, 32)), ("lift", (512, 0))])
def test_linear_split_hi_only_tier_vs_fp64(L, dev, mode, k):
    """hi_only = 1: only the hi halves of the operands are read and only the hi halves of Y are written - the lo halves of a sentinel-filled
    Y come back bit for bit.  The hi halves alone are held to the hi-only bound, colmax (from the f32 accumulators) too."""
    c = Case(L, dev, M=3 * 384, N=256, K0=k[0], K1=k[1], rpg=384, valid=300, mode=mode, bias="strided", relu_out=int(mode != "dual"),
             seed=7, hi_only=True)
    Y, cm = c.run(y_fill=SENTINEL)
    hi, lo = _halves(Y)
    assert bool((lo == SENTINEL).all()), f"hi-only {mode}: {int((lo != SENTINEL).sum())} lo halves written"
    got = hi.view(torch.float16).double()
    rows = torch.arange(c.M, device=dev)
    ref, tol = c.reference(rows)
    r = _ratio((got - ref).abs(), tol)
    assert r <= 1.0, f"hi-only {mode}: Y off by {r:.2f} x the bound"
    rc = _check_colmax(c, cm, tag=f"hi-only {mode}")
    print(f"[hi-only {mode} K={k}] max err/bound Y = {r:.3f}, colmax = {rc:.3f}")


# --------------------------------------------------------------------------------------------- tile schedule
def _schedule_case(cus, name):
    """(M, N, expected xcd_order) of a schedule case, sized from the CU count the way ehm_linear_split sizes its grid"""
    S = 2 * cus
    return {
        "fallback_small": (LBM * 5, 3 * LBN, False),                 # 15 tiles: G = 15, not a multiple of 8
        "xcd_small": (LBM * 8, 2 * LBN, True),                       # 16 tiles, n_tiles = 2: G = 16, per = 1
        "exact_grid": (LBM * cus, 2 * LBN, True),                    # tiles == 2 CUs: one tile per block
        "grid_plus_one": (LBM * (S + 1), LBN, True),                 # tiles == 2 CUs + 1: block 0 takes a second tile
        "xcd_ragged_n1": (LBM * (S + S // 3 + 5), LBN, True),        # n_tiles = 1: rounds of 8 per = 2 CUs row tiles, the last one ragged
        "xcd_ragged_n2": (LBM * (cus + cus // 6 + 3), 2 * LBN, True),  # n_tiles = 2: rounds of CUs row tiles, the last one ragged
        "fallback_n3": (LBM * (S // 3 + 29), 3 * LBN, False),        # n_tiles = 3 (N = 384): (G / 8) % 3 != 0, several tiles per block
    }[name]


@pytest.mark.parametrize("name", ["fallback_small", "xcd_small", "exact_grid", "grid_plus_one", "xcd_ragged_n1", "xcd_ragged_n2", "fallback_n3"])
def test_linear_split_tile_schedule_vs_fp64(L, dev, cus, name):
    """Both tile orders of the persistent grid (tile_of): the XCD-grouped order (G % 8 == 0 and (G / 8) % n_tiles == 0) and the linear
    fallback, with one tile per block, one block taking a second tile, and ragged last rounds.  The branch each case takes is asserted
    from the device's CU count, so another CU count cannot silently change what is tested."""
    M, N, want_xcd = _schedule_case(cus, name)
    G, xcd = _schedule(cus, M, N)
    m_tiles, n_tiles = M // LBM, N // LBN
    assert xcd == want_xcd, (name, cus, G, xcd)
    per_block = [len(_tiles_of(b, G, xcd, m_tiles, n_tiles)) for b in range(G)]
    assert sum(per_block) == m_tiles * n_tiles
    if name == "exact_grid":
        assert G == m_tiles * n_tiles and set(per_block) == {1}
    if name == "grid_plus_one":
        assert G == 2 * cus and sorted(per_block)[-2:] == [1, 2] and per_block.count(2) == 1
    if name.startswith("xcd_ragged"):
        per = (G // 8) // n_tiles
        assert G == 2 * cus and m_tiles % (8 * per) != 0 and len(set(per_block)) == 2
    if name == "fallback_n3":
        assert G == 2 * cus and max(per_block) >= 2
    c = Case(L, dev, M=M, N=N, K0=64, K1=32, rpg=LBM, mode="dual", bias="strided", relu_out=0, seed=31)
    Y, cm = c.run()
    r = _check_y(c, Y, tag=f"schedule {name}")
    rc = _check_colmax(c, cm, tag=f"schedule {name}")
    print(f"[schedule {name}: M={M} N={N} G={G} xcd={xcd}] max err/bound Y = {r:.3f}, colmax = {rc:.3f}")


def test_linear_split_pointnet_sized_launch_vs_fp64(L, dev, cus):
    """The benchmark's PointNet launch shape: 256 bodies x 4224 padded points (4100 valid), N = 256, the dual-source fc_1 + shortcut GEMM
    (K = 256 + 256) with the strided per-body bias and colmax.  Y is checked on sampled row tiles - among them the first and last row
    tiles of the blocks' final iteration and both sides of a group boundary - and colmax on every group."""
    B, Np, nv = 256, 4224, 4100
    M, N = B * Np, 256
    G, xcd = _schedule(cus, M, N)
    assert xcd, (cus, G)
    c = Case(L, dev, M=M, N=N, K0=256, K1=256, rpg=Np, valid=nv, mode="dual", bias="strided", relu_out=0, seed=41)
    Y, cm = c.run()
    m_tiles = M // LBM
    last = [_tiles_of(b, G, xcd, m_tiles, 2)[-1][0] for b in range(G)]
    sample = {0, 1, Np // LBM - 1, Np // LBM, m_tiles - 1, min(last), max(last), last[0], last[-1]}
    sample |= set(torch.randint(0, m_tiles, (24,), generator=torch.Generator().manual_seed(5)).tolist())
    rows = torch.cat([torch.arange(m * LBM, (m + 1) * LBM) for m in sorted(sample)]).to(dev)
    Yf = torch.empty(rows.numel(), N, device=dev)
    for i, m in enumerate(sorted(sample)):
        Yf[i * LBM:(i + 1) * LBM] = _unx2(L, Y, LBM, m * LBM)
    ref, tol = c.reference(rows)
    r = _ratio((Yf.double() - ref).abs(), tol)
    assert torch.isfinite(Yf).all() and r <= 1.0, r
    del Y
    rc = _check_colmax(c, cm, tag="pointnet-sized")
    print(f"[pointnet-sized M={M} G={G}] {len(sample)} row tiles, max err/bound Y = {r:.3f}, colmax = {rc:.3f}")


# --------------------------------------------------------------------------------------------- groups, valid rows, colmax semantics
def test_linear_split_many_groups_of_one_tile(L, dev):
    """rows_per_group = 192: every row tile is its own group (64 groups, 150 valid rows each: every tile takes the recomputed maximum)."""
    c = Case(L, dev, M=64 * 192, N=256, K0=256, rpg=192, valid=150, mode="relu_in0", bias="dense", relu_out=1, seed=51)
    Y, cm = c.run()
    r, rc = _check_y(c, Y, tag="rpg 192"), _check_colmax(c, cm, tag="rpg 192")
    print(f"[rpg 192 x 64 groups] max err/bound Y = {r:.3f}, colmax = {rc:.3f}")


@pytest.mark.parametrize("valid", [1, 95, 96, 97, 191, 192, 200, 575])
@pytest.mark.parametrize("mode", ["plain", "lift"])
def test_linear_split_valid_rows_of_a_group(L, dev, valid, mode):
    """rows_per_group = 576 (three row tiles) with valid rows that end inside the first wave's 96 rows, on its boundary, inside the second
    wave, on a tile boundary, and one short of the group.  The rows past `valid` of A hold large values: a single one of them in colmax
    shows.  (Lift mode generates its padding rows from zero points instead.)"""
    c = Case(L, dev, M=4 * 576, N=128, K0=96, rpg=576, valid=valid, mode=mode, bias="bias", relu_out=0, seed=valid)
    Y, cm = c.run()
    r, rc = _check_y(c, Y, tag=f"valid {valid}"), _check_colmax(c, cm, tag=f"valid {valid} {mode}")
    print(f"[valid {valid}/576 {mode}] max err/bound Y = {r:.3f}, colmax = {rc:.3f}")


def test_linear_split_colmax_of_all_negative_outputs(L, dev):
    """relu_out = 0 and a strongly negative bias: every output is negative, so every colmax update takes the atomicMin branch of
    atomic_max_float (on -inf, then on negative values)."""
    c = Case(L, dev, M=4 * 384, N=256, K0=128, rpg=384, valid=333, mode="plain", bias="bias", relu_out=0, seed=61)
    c.bias -= 1000.0
    Y, cm = c.run()
    assert bool((cm < -900).all())
    r, rc = _check_y(c, Y, tag="negative"), _check_colmax(c, cm, tag="negative")
    print(f"[all negative] max err/bound Y = {r:.3f}, colmax = {rc:.3f}")


def test_linear_split_colmax_of_an_all_zero_column_is_plus_zero(L, dev):
    """relu_out = 1 with every output rectified to zero: Y is all zero and colmax is +0.0 (bits 0), not -inf or -0.0."""
    c = Case(L, dev, M=2 * 384, N=128, K0=64, rpg=384, valid=200, mode="relu_in0", bias="bias", relu_out=1, seed=62)
    c.bias -= 1000.0
    Y, cm = c.run()
    assert bool((_unx2(L, Y) == 0).all())
    assert bool((cm.view(torch.int32) == 0).all()), cm


def test_linear_split_colmax_into_a_prefilled_running_max(L, dev):
    """colmax is a running maximum: prefilled values above a column's outputs stay (bit for bit), lower ones are replaced.  Prefills of
    both signs over columns of both signs (bias +-3: positive outputs meet negative prefills and the reverse)."""
    c = Case(L, dev, M=3 * 384, N=256, K0=96, rpg=384, valid=250, mode="plain", bias="bias", relu_out=0, seed=63)
    c.bias.copy_(torch.where(torch.arange(256, device=dev) % 2 == 0, 3.0, -3.0))
    ref, _ = c.colmax_reference()
    g = torch.Generator(device=dev).manual_seed(64)
    offs = torch.where(torch.rand(ref.shape, generator=g, device=dev) < 0.5, -1.0, 1.0) * (0.5 + torch.rand(ref.shape, generator=g, device=dev))
    prefill = (ref + offs).float()                            # half the columns above their max, half below
    prefill[0, :8] = -0.0
    prefill[1, :8] = float("-inf")
    Y, cm = c.run(prefill=prefill)
    kept = prefill.double() > ref
    assert torch.equal(cm[kept], prefill[kept])
    rc = _check_colmax(c, cm, prefill=prefill, tag="prefill")
    print(f"[prefilled colmax] {int(kept.sum())} of {kept.numel()} kept, max err/bound = {rc:.3f}")


def test_linear_split_is_deterministic(L, dev):
    c = Case(L, dev, M=8 * 576, N=256, K0=256, K1=32, rpg=576, valid=500, mode="dual", bias="strided", relu_out=0, seed=65)
    Y1, cm1 = c.run()
    Y2, cm2 = c.run()
    assert torch.equal(Y1.view(torch.int32), Y2.view(torch.int32)) and torch.equal(cm1.view(torch.int32), cm2.view(torch.int32))


def test_linear_split_range_behaviour(L, dev):
    """Outside the f16 range.  An element of A at 7e4 (> 65504: hi saturates, lo carries the remaining 4496, still represented) and one at
    2e5 (both halves saturate: it reads as 131008, the format's limit).  Output columns driven to +-2e5 and to 1e5 by their bias: Y
    saturates at +-131008 (hi at 65504, lo the rest, stored exactly only up to the f16 precision of lo) and stays finite, colmax takes the
    unclamped float32 value, nothing is inf or NaN.  The engine has no range flag (the GCN and conv have one); this pins what it does."""
    c = Case(L, dev, M=2 * 384, N=256, K0=128, rpg=384, valid=300, mode="plain", bias="bias", relu_out=0, seed=71)
    c.A0[5, 17] = 7e4
    c.A0[400, 3] = 2e5
    c.A0x2 = _x2(L, c.A0)
    c.bias[10], c.bias[11], c.bias[12] = 2e5, -2e5, 1e5
    Y, cm = c.run()
    got = _unx2(L, Y).double()
    assert torch.isfinite(got).all() and torch.isfinite(cm).all()
    c.A0[400, 3] = 131008.0                                   # the value the format holds
    rows = torch.arange(c.M, device=dev)
    ref, tol = c.reference(rows)
    big = ref.abs() >= 65504
    assert bool(big[:, 10].all() and big[:, 11].all() and big[:, 12].all())
    exp = ref.clamp(-131008.0, 131008.0)
    # past 65504 the model's |lo| <= 2^-11 |x| no longer holds: lo carries the excess |x| - 65504 at f16 precision.  In A that makes the dropped
    # lo . wl product and the rounding of lo each up to 2^-11 excess |w|; in Y the stored lo is off by up to 2^-11 (|y| - 65504)
    excess = (c.A0.double().abs() - 65504).clamp_min(0)
    tol = tol + 2 * 2.0 ** -11 * (excess @ c.W.double().abs().t())
    valid = ((rows % c.rpg) < c.nv)[:, None]
    cm_ref = torch.where(valid, ref, -math.inf).view(c.groups, c.rpg, c.N).max(1).values
    cm_tol = torch.where(valid, tol, 0.0).view(c.groups, c.rpg, c.N).max(1).values
    tol = torch.where(big, 2.0 ** -11 * (ref.abs() - 65504).clamp_min(0) + tol, tol)
    r = _ratio((got - exp).abs(), tol)
    assert r <= 1.0, r
    assert float(got[:, 10].min()) == 131008.0 and float(got[:, 11].max()) == -131008.0
    rc = _ratio((cm.double() - cm_ref).abs(), cm_tol)
    assert rc <= 1.0, rc
    assert float(cm[:, 10].min()) > 190000.0                   # unclamped
    print(f"[range] max err/bound Y = {r:.3f}, colmax = {rc:.3f}")


def test_linear_split_offsets_beyond_2_gib(L, dev):
    """M = 192 x 11200 rows, K0 = N = 256: the A0 and Y matrices are 2.2 GB each, so the last row tiles' bases lie past 2^31 bytes (the
    engine forms a 64-bit base per tile in its buffer descriptors).  First, middle and last row tiles against float64."""
    M, N, K0 = 192 * 11200, 256, 256
    assert M * K0 * 4 > 2 ** 31
    c = Case(L, dev, M=M, N=N, K0=K0, rpg=192 * 1400, mode="plain", bias="bias", relu_out=1, seed=81)
    Y, _ = c.run(colmax=False)
    m_tiles = M // LBM
    tiles = [0, m_tiles // 2, m_tiles - 2, m_tiles - 1]
    assert (m_tiles - 1) * LBM * K0 * 4 > 2 ** 31
    rows = torch.cat([torch.arange(m * LBM, (m + 1) * LBM) for m in tiles]).to(dev)
    got = torch.cat([_unx2(L, Y, LBM, m * LBM) for m in tiles]).double()
    ref, tol = c.reference(rows)
    r = _ratio((got - ref).abs(), tol)
    assert torch.isfinite(got).all() and r <= 1.0, r
    print(f"[beyond 2 GiB] max err/bound = {r:.3f}")
    del Y, c
    torch.cuda.empty_cache()


# --------------------------------------------------------------------------------------------- companion kernels
@pytest.mark.parametrize("K", [32, 1024, 1056])          # 1056: the 16-wave path with an uneven K split
@pytest.mark.parametrize("M", [1, 33, 256])
def test_skinny_gemm_rectified_leading_columns_vs_fp64(dev, M, K):
    """ehm_skinny_gemm_f32 with relu = (c << 1) | r: the INPUT of the first c output columns is rectified (c in {0, 32, N}), r rectifies
    the output.  Exact float32 (an fma chain per wave, then the waves' partial sums): |err| <= (K / NW + NW + 10) 2^-24 S with
    S = |X'| . |W| + |b| - the rigorous worst case."""
    from egohmr_amd import _lib
    L = _lib.lib()
    N = 96
    g = torch.Generator(device=dev).manual_seed(M * 7 + K)
    X, W, b = torch.randn(M, K, generator=g, device=dev), torch.randn(K, N, generator=g, device=dev) / K ** 0.5, torch.randn(N, generator=g, device=dev)
    NW = 16 if K >= 1024 else 4
    worst = 0.0
    for cols in (0, 32, N):
        for r in (0, 1):
            Xp = X.double().clone().expand(N, M, K).clone()            # per output column: the input it sees
            Xp[:cols] = torch.relu(Xp[:cols])
            ref = torch.einsum("nmk,kn->mn", Xp, W.double()) + b.double()
            S = torch.einsum("nmk,kn->mn", Xp.abs(), W.double().abs()) + b.double().abs()
            if r:
                ref = ref.clamp_min(0)
            Y = torch.full((M, N), float("nan"), device=dev)
            _check(L.ehm_skinny_gemm_f32(X.data_ptr(), W.data_ptr(), b.data_ptr(), Y.data_ptr(), M, K, N, (cols << 1) | r, None), L)
            torch.cuda.synchronize()
            tol = (K / NW + NW + 10) * 2.0 ** -24 * S
            ratio = _ratio((Y.double() - ref).abs(), tol)
            assert ratio <= 1.0, (cols, r, ratio)
            worst = max(worst, ratio)
    print(f"[skinny M={M} K={K}] max err/bound = {worst:.3f}")


@pytest.mark.parametrize("groups", [1, 256])
@pytest.mark.parametrize("C_", [32, 2048])
@pytest.mark.parametrize("hw", [1, 49])
def test_x2_group_mean_vs_fp64(L, dev, hw, C_, groups):
    """ehm_x2_group_mean (the ResNet's average pool) on X2 input, split and hi-only.  Split: |err| <= (2^-22 + (hw + 2) 2^-24) mean|x| + 2^-25.
    hi_only = 1 must read the hi halves alone (the lo halves hold a large sentinel here): |err| <= (2^-11 + (hw + 2) 2^-24) mean|x| + 2^-25
    against the exact inputs, and the accumulation term alone against the mean of the hi halves."""
    g = torch.Generator(device=dev).manual_seed(hw * 3 + C_ + groups)
    rows = groups * hw
    X = torch.randn(rows + 192, C_, generator=g, device=dev)
    X[rows:] = 1e3                                            # rows past the groups must not be read
    X2 = _x2(L, X)
    ref = X[:rows].double().view(groups, hw, C_).mean(1)
    mabs = X[:rows].double().abs().view(groups, hw, C_).mean(1)
    acc = (hw + 2) * 2.0 ** -24 * mabs
    Y = torch.full((groups, C_), float("nan"), device=dev)
    _check(L.ehm_x2_group_mean(X2.data_ptr(), Y.data_ptr(), groups, hw, C_, 0, None), L)
    torch.cuda.synchronize()
    r_split = _ratio((Y.double() - ref).abs(), 2.0 ** -22 * mabs + acc + 2.0 ** -25)
    assert r_split <= 1.0, r_split
    X2.view(torch.int16).view(-1, C_ // 32, 2, 32)[:, :, 1, :] = 0x6000      # f16 512.0 in every lo half
    hi_mean = _halves(X2)[0][:rows].view(torch.float16).double().view(groups, hw, C_).mean(1)
    Y.fill_(float("nan"))
    _check(L.ehm_x2_group_mean(X2.data_ptr(), Y.data_ptr(), groups, hw, C_, 1, None), L)
    torch.cuda.synchronize()
    r_hi = _ratio((Y.double() - ref).abs(), 2.0 ** -11 * mabs + acc + 2.0 ** -25)
    r_hi_only = _ratio((Y.double() - hi_mean).abs(), acc + 2.0 ** -40)
    assert r_hi <= 1.0 and r_hi_only <= 1.0, (r_hi, r_hi_only)
    print(f"[group mean hw={hw} C={C_} groups={groups}] max err/bound split = {r_split:.3f}, hi-only = {r_hi:.3f} / {r_hi_only:.3f}")


@pytest.mark.parametrize("bodies", [1, 300])
@pytest.mark.parametrize("Ci", [32, 64, 96, 512])
def test_nonlocal_attention_vs_fp64(dev, Ci, bodies):
    """ehm_nonlocal_attention: y = softmax(theta phi^T) g per body of 24 joints, with logits of standard deviation 40 (the largest past 89,
    where exp overflows float32: the max-subtraction must be there), Ci % 64 != 0 (the last 64-channel slab ragged).  Error model: a logit is an f32 fma chain over Ci
    channels, error <= 4 sqrt(Ci) 2^-24 (|l| + 4 r) with r = sqrt(sum theta^2 phi^2) (random-signed terms); a logit error d moves y by at most
    max|d| sum_b P_ab |g_b - y_a| (first order, doubled here); exp, normalisation and the 24-term sum add 64 2^-24 sum_b P_ab |g_b|."""
    from egohmr_amd import _lib
    L = _lib.lib()
    g = torch.Generator(device=dev).manual_seed(Ci + bodies)
    rows = bodies * 24
    a = (40.0 / math.sqrt(Ci)) ** 0.5
    qkv = torch.cat([torch.randn(rows, Ci, generator=g, device=dev) * a, torch.randn(rows, Ci, generator=g, device=dev) * a,
                     torch.randn(rows, Ci, generator=g, device=dev)], 1).contiguous()
    th, ph, gv = (qkv[:, i * Ci:(i + 1) * Ci].double().view(bodies, 24, Ci) for i in range(3))
    logit = th @ ph.transpose(1, 2)
    assert float(logit.abs().max()) > 89.0                    # exp overflows float32 without the max-subtraction
    P = torch.softmax(logit, -1)
    ref = P @ gv
    r_l = torch.sqrt((th * th) @ (ph * ph).transpose(1, 2))
    dl = (4 * math.sqrt(Ci) * 2.0 ** -24 * (logit.abs() + 4 * r_l)).amax(-1, keepdim=True)
    spread = (P[..., None] * (gv[:, None, :, :] - ref[:, :, None, :]).abs()).sum(2)
    tol = 2 * dl * spread + 64 * 2.0 ** -24 * (P @ gv.abs())
    y = torch.full((rows, Ci), float("nan"), device=dev)
    _check(L.ehm_nonlocal_attention(qkv.data_ptr(), y.data_ptr(), bodies, Ci, None), L)
    torch.cuda.synchronize()
    got = y.double().view(bodies, 24, Ci)
    assert torch.isfinite(got).all()
    r = _ratio((got - ref).abs(), tol)
    assert r <= 1.0, r
    print(f"[non-local Ci={Ci} bodies={bodies}] |logit|max = {float(logit.abs().max()):.1f}, max err/bound = {r:.3f}")


@pytest.mark.parametrize("scale", [1.0, 1024.0])
@pytest.mark.parametrize("K,Kp", [(40, 64), (32, 96), (257, 288), (64, 64)])
def test_split_pack_round_trip(L, dev, K, Kp, scale):
    """ehm_split_pack -> X2 [rows, Kp]: hi = f16(x s), lo = f16(x s - hi) bit for bit (|x s - hi - lo| <= 2^-22 |x s| + 2^-25), the padding
    columns K..Kp zero; ehm_gcn_unpack_activations returns hi + lo."""
    rows = 1000
    g = torch.Generator(device=dev).manual_seed(K + Kp)
    X = torch.randn(rows, K, generator=g, device=dev) * torch.logspace(-6, 1, K, device=dev)[None]
    X[0, 0], X[1, 0] = 60000.0 / scale, -1e-7
    out = torch.empty(rows, Kp, device=dev).fill_(float("nan"))
    _check(L.ehm_split_pack(X.data_ptr(), out.data_ptr(), rows, K, Kp, scale, None), L)
    xs = X * scale
    hi_x = xs.cpu().clamp(-65504, 65504).half()                                # (round to nearest even, f16 subnormals kept)
    lo_x = (xs.cpu() - hi_x.float()).clamp(-65504, 65504).half()
    hi, lo = _halves(out)
    assert torch.equal(hi[:, :K].cpu(), hi_x.view(torch.int16)) and torch.equal(lo[:, :K].cpu(), lo_x.view(torch.int16))
    assert bool((hi[:, K:] == 0).all() and (lo[:, K:] == 0).all())
    back = _unx2(L, out).double()
    torch.cuda.synchronize()
    assert bool((back[:, K:] == 0).all())
    err = (back[:, :K] - xs.double()).abs()
    assert bool((err <= 2.0 ** -22 * xs.double().abs() + 2.0 ** -25).all()), float(err.max())


@pytest.mark.parametrize("B,N,Np", [(3, 300, 331), (2, 5, 192), (1, 128, 128)])
def test_pointnet_lift_vs_fp64(L, dev, B, N, Np):
    """ehm_pointnet_lift: R0 = relu(p Wpos^T + b) (an fma chain: |err| <= 3 2^-24 (|p||Wpos| + |b|), then the split: 2^-22 |R0| + 2^-25) and
    P32 = the points in columns 0..2, zero elsewhere, both X2, on a ragged N_padded (B * Np rows, not a multiple of the kernel's 8 rows per
    block).  Padding rows: P32 zero, R0 = relu(b) (zero points)."""
    C0 = 512
    g = torch.Generator(device=dev).manual_seed(N + Np)
    pts = torch.rand(B, N, 3, generator=g, device=dev) * 2 - 1
    Wpos, bpos = torch.randn(C0, 3, generator=g, device=dev) * 0.7, torch.randn(C0, generator=g, device=dev) * 0.3
    rows = B * Np
    R0 = torch.full((rows, C0), float("nan"), device=dev)
    P32 = torch.full((rows, 32), float("nan"), device=dev)
    _check(L.ehm_pointnet_lift(pts.data_ptr(), Wpos.data_ptr(), bpos.data_ptr(), R0.data_ptr(), P32.data_ptr(), B, N, Np, C0, None), L)
    p = torch.zeros(B, Np, 3, dtype=torch.float64, device=dev)
    p[:, :N] = pts.double()
    p = p.view(rows, 3)
    ref = torch.relu(p @ Wpos.double().t() + bpos.double())
    tol = 3 * 2.0 ** -24 * (p.abs() @ Wpos.double().abs().t() + bpos.double().abs()) + 2.0 ** -22 * ref.abs() + 2.0 ** -25
    got = _unx2(L, R0).double()
    r = _ratio((got - ref).abs(), tol)
    assert torch.isfinite(got).all() and r <= 1.0, r
    got_p = _unx2(L, P32).double()
    assert torch.equal(got_p[:, 3:], torch.zeros_like(got_p[:, 3:]))
    pad = (torch.arange(rows, device=dev) % Np) >= N
    assert bool((_halves(P32)[0][pad] == 0).all() and (_halves(P32)[1][pad] == 0).all())
    assert bool(((got_p[:, :3] - p).abs() <= 2.0 ** -22 * p.abs() + 2.0 ** -25).all())
    print(f"[pointnet lift B={B} N={N} Np={Np}] max err/bound R0 = {r:.3f}")
