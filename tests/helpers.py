"""shared helpers of the test-suite (oracle-side set-up)"""
import numpy as np

from oracle.grid import default_axes
from oracle.model import Iage, Py2dModel


def oracle_iage(nz, ny, max_abs_vvel=0.1, horiz_mix_coeff=1000.0):
    depth, ypos = default_axes(nz, ny)
    model = Py2dModel(depth, ypos, max_abs_vvel, horiz_mix_coeff)
    return model, Iage(model)


def rel_err(a, b):
    a = np.asarray(a)
    b = np.asarray(b)
    den = np.max(np.abs(b))
    return float(np.max(np.abs(a - b)) / (den if den > 0 else 1.0))


def free_years(eng, x, **kw):
    """one free-running forward year with SciPy's controller decision for decision (Jacobian reuse of
    radau.py:509-517, no memory of Newton failures: the mode whose counters are comparable with solve_ivp's)
    and one in the engine's default mode (Jacobian re-evaluated for every step attempt, at its second stage time
    after a Newton failure): ((fx, stats, sched), (fx, stats, sched))"""
    from nk_ooc_amd.engine import DEFAULT_GROWTH_CAP, DEFAULT_JAC_FRESH, DEFAULT_JAC_STAGE

    eng.set_option("jac_fresh", 0)
    eng.set_option("growth_cap", 0)
    eng.set_option("jac_stage", -1)
    try:
        faithful = eng.comp_fcn(x, **kw)
    finally:
        eng.set_option("jac_fresh", DEFAULT_JAC_FRESH)
        eng.set_option("growth_cap", DEFAULT_GROWTH_CAP)
        eng.set_option("jac_stage", DEFAULT_JAC_STAGE)
    return faithful, eng.comp_fcn(x, **kw)


def oracle_module(nz, ny, module=None):
    """the oracle's tracer module on the default nz x ny grid from a picklable description: None (iage), or a dict with
    "kind" ("iage", "phosphorus", "forced"), "params" (keyword arguments of the module: the phosphorus parameters, the
    options of oracle.model.Forced) and "forcing" (the (times, values) series of the file-driven forced options, by keyword)"""
    from oracle.model import Forced, Phosphorus

    model, iage = oracle_iage(nz, ny)
    kind = "iage" if module is None else module["kind"]
    params = {} if module is None else dict(module.get("params") or {})
    forcing = {} if module is None else dict(module.get("forcing") or {})
    if kind == "iage":
        return iage
    if kind == "phosphorus":
        return Phosphorus(model, **params)
    if kind == "forced":
        return Forced(model, **params, **{name: (np.asarray(t), np.asarray(v)) for name, (t, v) in forcing.items()})
    raise ValueError(f"unknown oracle module kind {kind!r}")


def oracle_year_job(args):
    """one CPU year of the oracle on one BLAS thread, for worker processes of the parity tests (spawned: they never touch
    the GPU): args = (nz, ny, x, rows[, module]) -- a replay of the accepted steps `rows` from x, or (rows None) a
    free-running year; of iage, or of the module that `oracle_module` makes of the description `module`"""
    from threadpoolctl import threadpool_limits

    from oracle import radau

    nz, ny, x, rows = args[:4]
    tm = oracle_module(nz, ny, args[4] if len(args) > 4 else None)
    with threadpool_limits(limits=1):
        if rows is None:
            return radau.comp_fcn(tm, x)
        return radau.comp_fcn(tm, x, replay=rows)


# ---- the preconditioner's dense kernels at every block-size class (test_precond_blocks_host.py on the CPU,
# test_gpu_precond_blocks.py on the device: one set of grids and shifts, so the two cannot drift) ----------------------
YEAR = 365.0 * 86400.0
# group 1, shifted systems of a one-tracer forced module (block size m = nz): a single partial panel (m < 32) and a single
# tile (32 < m < 64); m a multiple of 32 or 64 (full last panel, exact tiles); m = 1 mod 32 (a last panel of one pivot); the
# next pivot block in the first and in the second half of a tile at a ragged edge (97, 129, 160, 193); odd m (the general
# mat-vec).  ny = 2: empty right chain of the two-ended elimination; ny = 5: unequal chains with an inward mat-vec
FORCED_MODELINFO = {"forced_surf_restore_opt": "none", "forced_sms_opt": "decay", "forced_sms_decay_rate": "1.0e-8"}
FORCED_DECAY_RATE = 1.0e-8
SHIFT_TIME = 0.5 * YEAR
FORCED_SHIFT_GRIDS = [(nz, ny) for nz in (2, 3, 16, 31, 32, 33, 63, 64, 65, 96, 97, 128, 129, 160, 193) for ny in (2, 5)]
FORCED_SHIFTS = [0.02, -0.03]
# group 2, shifted systems of iage (m = 2 nz).  Shifts kept after the host twin was run on them: 0.02 and 0.5 (twin against
# splu <= 1e-10 on every grid, asserted by test_precond_blocks_host.py); -0.03 was NOT kept -- the slowly restored tracer
# brings the operator's condition number to 5e11 there, and no sparse LU is a reference at 1e-8 for that
IAGE_SHIFT_GRIDS = [(nz, ny) for nz in (16, 32, 33, 64, 65, 96) for ny in (2, 3)]
IAGE_SHIFTS = [0.02, 0.5]
# group 3, the time-periodic system of iage (m = 3 nz = 6, 33, 96, 129, 192, 255, 258)
PERIODIC_GRIDS = [(2, 2), (11, 3), (32, 2), (43, 3), (64, 2), (85, 3), (86, 2)]
# group 4, rows longer than one mat-vec chunk of 1280 columns: m = 1281 (odd: the general kernel), 1284 (the second chunk
# holds two double2; ny = 5 so that the two-ended inward pair runs long rows too), 1536 (the largest block the library takes)
LONG_ROW_GRIDS = [(427, 2), (428, 5), (512, 2)]
SHIFT_BAR = 1e-8        # test_phosphorus_preconditioner's bar for shifted solves
PERIODIC_BAR = 1e-9     # test_precond_apply's bar
TWIN_BAR = 1e-10        # the host twin against the sparse reference: two decades (one at 1e-9) below the device's bars


def oracle_shift_module(kind, nz, ny):
    """the oracle's module of the shifted-system groups on the default grid: "forced" (one tracer, decay) or "iage" """
    from oracle.model import Forced

    model, iage = oracle_iage(nz, ny)
    return Forced(model, "none", 0.0, "decay", FORCED_DECAY_RATE) if kind == "forced" else iage


def shifted_operator(module, sigma):
    """YEAR J(YEAR / 2) - sigma I of a state independent module, CSC, unknowns in the state vector's order (tracer, depth, ypos)"""
    from scipy import sparse

    jac = module.comp_jacobian(SHIFT_TIME)
    return (YEAR * jac - sigma * sparse.identity(jac.shape[0])).tocsc()


def column_blocks(tc, nz, ny):
    """unknowns of the shifted systems by ypos column, (tracer, depth) inside a block as the library orders them"""
    base = (np.arange(tc * nz) * ny)
    return [base + j for j in range(ny)]


def periodic_operator(module, time_range=(0.0, YEAR), time_n=3):
    """the time-periodic block system of oracle.model.apply_precond_stable (state independent modules), CSC"""
    from scipy import sparse

    jac0 = module.comp_jacobian(0.0)
    n = jac0.shape[0]
    dt = (time_range[1] - time_range[0]) / time_n
    eye = sparse.identity(n, format="csr")
    rows = []
    for k in range(time_n):
        row = [None] * time_n
        row[k] = eye - dt * module.comp_jacobian(time_range[0] + (k + 0.5) * dt)
        row[(k - 1) % time_n] = -eye
        rows.append(row)
    return sparse.bmat(rows, format="csc")


def block_tridiag_solve(mat, blocks, rhs):
    """The library's algorithm on the host (csrc/nk2d_precond.hip), dense NumPy in float64: block-tridiagonal elimination
    over `blocks` (index arrays of the unknowns of each block; `mat` couples neighbouring blocks only) with EXPLICIT
    inverses of the Schur complements S_j = D_j - L_j S_{j-1}^-1 U_{j-1}, then y_j = r_j - L_j S_{j-1}^-1 y_{j-1} and
    x_j = S_j^-1 (y_j - U_j x_{j+1}).  Returns the solution on the unknowns of `blocks` (zero elsewhere)."""
    mat = mat.tocsr()
    rows = [mat[idx] for idx in blocks]
    nb = len(blocks)
    sinv, y = [], []
    for j in range(nb):
        s = rows[j][:, blocks[j]].toarray()
        r = np.array(rhs[blocks[j]], dtype=np.float64)
        if j > 0:
            lo = rows[j][:, blocks[j - 1]]
            up = rows[j - 1][:, blocks[j]]
            s = s - lo @ (up.T @ sinv[j - 1].T).T       # L (S^-1 U): the couplings stay sparse
            r = r - lo @ (sinv[j - 1] @ y[j - 1])
        sinv.append(np.linalg.inv(s))
        y.append(r)
    out = np.zeros(mat.shape[0])
    x_next = None
    for j in range(nb - 1, -1, -1):
        r = y[j]
        if j < nb - 1:
            r = r - rows[j][:, blocks[j + 1]] @ x_next
        x_next = sinv[j] @ r
        out[blocks[j]] = x_next
    return out


def twin_shift_solve(module, sigma, v):
    """the host twin of nk2d_shift_factor / nk2d_shift_solve (mode 1): every tracer of a column in one block"""
    m = module.model
    return block_tridiag_solve(shifted_operator(module, sigma), column_blocks(module.tc, m.nz, m.ny), v)


def twin_precond_apply(module, v):
    """the host twin of nk2d_precond_setup / nk2d_precond_apply (mode 0): per tracer, a block is one ypos column at the
    three time levels (m = 3 nz); M^-1 v = -(u_3 + v)"""
    m = module.model
    n = module.tc * m.nz * m.ny
    big = periodic_operator(module)
    rhs = np.zeros(3 * n)
    rhs[:n] = v
    u = np.zeros(3 * n)
    for tr in range(module.tc):
        cells = (tr * m.nz + np.arange(m.nz)) * m.ny
        level = np.concatenate([tau * n + cells for tau in range(3)])
        u += block_tridiag_solve(big, [level + j for j in range(m.ny)], rhs)
    return -(u[2 * n:] + v)


def block_rhs(n, seed=5):
    v = np.random.default_rng(seed).standard_normal(n)
    v.setflags(write=False)
    return v


# ---- the region-weighted Krylov algebra at every column-depth class (test_region_algebra_host.py on the CPU,
# test_gpu_region_algebra.py on the device: one set of grids, regions and inputs, so the two cannot drift) -----------
# nz: every levels-per-lane count E = ceil(nz / 64) = 1 ... 8 of the kernels' template, columns that end inside a lane
# slot and columns that fill it (64, 512), and the smallest column the library takes; ny cycled over the list
ALGEBRA_NZ = (2, 63, 64, 65, 130, 200, 257, 321, 390, 416, 449, 512)
ALGEBRA_GRIDS = [(nz, (2, 5, 7)[i % 3]) for i, nz in enumerate(ALGEBRA_NZ)]
ALGEBRA_TC = (1, 2, 3)
# the final reduction over tc * ny wave tasks: fewer tasks (2) than one wave of the block of 256 threads has lanes, and a
# count (261) that is no multiple of 256
ALGEBRA_REDUCE_SHAPES = [(1, 20, 2), (3, 20, 87)]
# capacity edges: (n + 1) nreg <= 4096 of nk2d_mgs at nreg = 64, n <= 512 of nk2d_multi_dot / multi_axpy / lin_comb
ALGEBRA_MGS_EDGE = (2, 20, 64)
ALGEBRA_N_EDGE = (2, 20, 2)
ALGEBRA_HOST_SHAPES = [(20, 3, 2), (70, 5, 2)]      # (nz, ny, tc) at which the reference is held to the oracle
ALGEBRA_NVEC = 7                                    # dot operands: vector 0 against vectors 1 ... 6
U53 = 2.0 ** -53


def _compress(mask):
    """region numbers 1 ... n without gaps (a number no cell carries would be a region of weight sum 0)"""
    vals = np.unique(mask[mask > 0])
    out = np.zeros_like(mask)
    for new, old in enumerate(vals):
        out[mask == old] = new + 1
    return out


def region_cases(nz, ny):
    """named region layouts of an nz x ny grid, each an oracle.krylov.Regions (mask and weight zeroed where either is, as
    model_config.gen_grid_vars does):
      depth_split     three regions stacked in depth; the boundaries are at levels that are multiples of neither 64 nor of
                      the levels per lane, the upper one at another level in every column (cycling where ny exceeds the
                      levels there are): lanes of one wave disagree, and a lane holds cells of two regions
      patchwork       a pseudo-random assignment to 5 regions, about 10 % of the cells in none
      sparse_regions  a region present in column 0 only, a region of exactly one cell, the last column outside every region
      columns         region j + 1 is column j (the reference's CI case)
    weights: outer(dz, dy) of the default grid times a factor in [0.5, 2]; everything from fixed seeds"""
    from oracle.krylov import Regions

    depth, ypos = default_axes(nz, ny)
    rng = np.random.default_rng([20, nz, ny])
    weight = np.outer(depth.delta, ypos.delta) * rng.uniform(0.5, 2.0, (nz, ny))
    lev = np.arange(nz)[:, None]
    e = (nz + 63) // 64
    cand = [k for k in range(1, nz) if k % 64 != 0 and (e == 1 or k % e != 0)]
    b2 = next((k for k in cand if 4 * k >= 3 * nz), cand[-1])
    lower = [k for k in cand if k < b2]
    if lower:
        b1 = np.array([lower[(len(lower) // 2 + j) % len(lower)] for j in range(ny)])[None, :]
        split = 1 + (lev >= b1) + (lev >= b2)
    else:       # two levels: the one interior boundary there is, the regions shifted from column to column
        split = 1 + (lev + np.arange(ny)[None, :]) % 3
    patch = rng.integers(1, 6, (nz, ny))
    patch[rng.random((nz, ny)) < 0.1] = 0
    sparse = np.ones((nz, ny), dtype=np.int64)
    sparse[:, ny - 1] = 0
    lo = nz // 4
    sparse[lo:max(lo + 1, 3 * nz // 4), 0] = 2
    sparse[nz - 1, (ny - 1) // 2] = 3
    columns = np.broadcast_to(np.arange(1, ny + 1)[None, :], (nz, ny))
    masks = {"depth_split": split, "patchwork": patch, "sparse_regions": sparse, "columns": columns}
    return {name: Regions(_compress(np.array(m, dtype=np.int32)), weight) for name, m in masks.items()}


def algebra_vectors(tc, nz, ny, n=ALGEBRA_NVEC, seed=31):
    """n state vectors (flat, (tracer, depth, ypos)) with entries sign * 10**uniform(-1, 1): no term of a regional dot is
    small enough to hide inside the dot's bound (asserted by test_region_algebra_host.py)"""
    rng = np.random.default_rng([seed, tc, nz, ny])
    size = (n, tc * nz * ny)
    vecs = np.where(rng.random(size) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-1.0, 1.0, size)
    vecs.setflags(write=False)
    return vecs


def algebra_coefs(nreg, n, seed=37):
    """n rows of per-region scalars, same distribution as the vectors"""
    rng = np.random.default_rng([seed, nreg, n])
    return np.where(rng.random((n, nreg)) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-1.0, 1.0, (n, nreg))


def _exact_products(wn, a, b):
    """wn * a * b of finite float64 arrays as exact integers T and one exponent: the values are T * 2**ex"""
    mant, expo = zip(*(np.frexp(v) for v in (wn, a, b)))
    ints = [np.ldexp(m, 53).astype(np.int64).astype(object) for m in mant]      # |m| < 1: 53-bit integers, exact
    ex = expo[0].astype(np.int64) + expo[1] + expo[2] - 159
    low = int(ex.min())
    return (ints[0] * ints[1] * ints[2]) << (ex - low).astype(object), low


class algebra_reference:
    """The region-weighted algebra of csrc/nk2d_api.hip and csrc/nk2d_krylov.hip in plain NumPy, with none of
    oracle.krylov's algebra: vectors are flat float64 arrays (tracer, depth, ypos), region scalars arrays [nreg].

    Element-wise operations are float64 in the operation order the kernels document, so the device must reproduce them
    bit for bit.  `dot` is exact rational arithmetic (fractions.Fraction of integer mantissa products) on the float64
    normalised weights wn = w * (1 / sum_region(w)), formed as nk2d_set_region forms them: the sum in flat index order,
    then the reciprocal, then the product.

    The bound of a device dot.  The device forms each of the N_r terms of region r as fl(wn * fl(a * b)) -- two roundings,
    relative error at most 2u + u^2 with u = 2**-53 -- from the same float64 wn, and adds them in some order (lanes,
    wave tree, column partials, block tree: N_r - 1 additions at most N_r - 1 deep; adding the zeros of cells of other
    regions is exact).  By the standard bound for recursive summation in any order (Higham, Accuracy and Stability of
    Numerical Algorithms, section 4.2) the computed sum is sum_k t_k (1 + theta_k) with |theta_k| <= gamma_(N_r + 1)
    = (N_r + 1) u / (1 - (N_r + 1) u) (N_r - 1 additions and two roundings of the term), which is at most (N_r + 3) u
    while (N_r + 1) (N_r + 3) u <= 2, i.e. for every N_r below 10**8 -- so
        |got - exact| <= (N_r + 3) * 2**-53 * S_r,   S_r = sum |wn a b| over the cells of region r, all tracers,
    whatever the order.  `dot_excess` compares with exactly this, no factor on it; nothing here was tuned on a device."""

    def __init__(self, reg, tc):
        self.reg, self.tc = reg, int(tc)
        self.nreg = reg.nreg
        self.mask = reg.mask.reshape(-1)
        weight = reg.weight.reshape(-1)
        self.wn = np.zeros(weight.size)
        for r in range(1, self.nreg + 1):
            idx = np.nonzero(self.mask == r)[0]
            total = 0.0
            for val in weight[idx].tolist():
                total += val
            self.wn[idx] = (1.0 / total) * weight[idx]
        self.count = self.tc * np.array([np.count_nonzero(self.mask == r) for r in range(1, self.nreg + 1)])

    def planes(self, x):
        return np.asarray(x, dtype=np.float64).reshape(self.tc, self.mask.size)

    def bcast(self, vals, fill=1.0):
        """the value of a region scalar at every cell of a plane, `fill` where the mask is <= 0"""
        return np.where(self.mask > 0, np.asarray(vals, dtype=np.float64)[np.maximum(self.mask, 1) - 1], fill)

    def axpby(self, a, x, b, y):
        return (self.bcast(a) * self.planes(x) + self.bcast(b) * self.planes(y)).reshape(-1)

    def diff_scale(self, x, y, s):
        return ((self.planes(x) - self.planes(y)) * self.bcast(s)).reshape(-1)

    def scale(self, x, s):
        return (self.planes(x) * self.bcast(s)).reshape(-1)

    def mask_out(self, x):
        return np.where(self.mask != 0, self.planes(x), 0.0).reshape(-1)

    def lin_comb(self, coef, vecs):
        res = self.bcast(coef[0]) * self.planes(vecs[0])
        for c, v in zip(coef[1:], vecs[1:]):
            res = res + self.bcast(c) * self.planes(v)
        return res.reshape(-1)

    def multi_axpy(self, w, vecs, h, fill):
        res = self.planes(w)
        for c, v in zip(h, vecs):
            res = res - self.bcast(c, fill) * self.planes(v)
        return res.reshape(-1)

    def dot(self, a, b):
        """(exact, s, n): per region the exact dot and S_r = sum |wn a b| as Fractions, and the cell count N_r"""
        from fractions import Fraction

        terms, low = _exact_products(np.tile(self.wn, self.tc), np.asarray(a).reshape(-1), np.asarray(b).reshape(-1))
        mask = np.tile(self.mask, self.tc)
        unit = Fraction(2) ** low
        exact, s = [], []
        for r in range(1, self.nreg + 1):
            sel = terms[mask == r].tolist()
            exact.append(sum(sel) * unit)
            s.append(sum(abs(t) for t in sel) * unit)
        return exact, s, self.count

    def dot_terms(self, a, b):
        """|wn a b| per cell (float64, all tracers) and the tiled mask: for the input condition of the dots"""
        return np.abs(np.tile(self.wn, self.tc) * (np.asarray(a).reshape(-1) * np.asarray(b).reshape(-1))), \
            np.tile(self.mask, self.tc)

    @staticmethod
    def dot_bound(s, n):
        """(N_r + 3) 2**-53 S_r, exact"""
        from fractions import Fraction

        return [Fraction(int(nr) + 3, 2 ** 53) * sr for sr, nr in zip(s, n)]

    def dot_excess(self, got, ref):
        """max over the regions of |got - exact| / bound for a device result `got` [nreg] and ref = self.dot(a, b): the
        comparison itself is exact; <= 1 passes.  A region without cells has exact = bound = 0: its dot must be 0.0"""
        from fractions import Fraction

        exact, s, n = ref
        worst = 0.0
        for g, ex, bound in zip(np.asarray(got, dtype=np.float64).tolist(), exact, self.dot_bound(s, n)):
            if not np.isfinite(g):
                return float("inf")
            err = abs(Fraction(g) - ex)
            worst = max(worst, float(err / bound) if bound > 0 else (0.0 if err == 0 else float("inf")))
        return worst

    def mgs(self, w, basis):
        """modified Gram-Schmidt with the exact dots: h_i = fl(<w_i, v_i>), w_(i+1) = fl(w_i - fl(bcast(h_i) v_i)).
        Returns (h [n, nreg], w, hbound [n, nreg]); hbound is the dot's bound propagated through the projections:
        a device that computes h'_i = h_i + e_i works on w'_i = w_i + d_i from then on.  With D_i >= |d_i| per cell
        (D_0 = 0) and E_i >= |e_i| per region,
            E_i = (N + 3) u (S(w_i, v_i) + G_i) + G_i + u |h_i|,      G_i = sum wn D_i |v_i| over the region
        (the device's dot of w'_i within its bound, whose S is at most S(w_i, v_i) + G_i; the exact dot of d_i; the
        rounding of h_i), and, both updates rounding a product and a difference,
            D_(i+1) = D_i + E_i |v_i| + u (1 + u) (2 |w_i| + D_i + 4 |h_i v_i| + 2 E_i |v_i|)
        (cells of no region: bcast is 1.0 on both sides and the same arithmetic, D stays 0 there)."""
        wn = np.tile(self.wn, self.tc)
        mask = np.tile(self.mask, self.tc)
        owned = mask > 0
        region = np.maximum(mask, 1) - 1
        w = np.array(w, dtype=np.float64).reshape(-1)
        dev = np.zeros(w.size)
        h = np.empty((len(basis), self.nreg))
        hbound = np.empty((len(basis), self.nreg))
        for i, v in enumerate(basis):
            v = np.asarray(v, dtype=np.float64).reshape(-1)
            exact, s, n = self.dot(w, v)
            h[i] = [float(x) for x in exact]
            g = np.bincount(region[owned], weights=(wn * dev * np.abs(v))[owned], minlength=self.nreg)
            sf = np.array([float(x) for x in s])
            hbound[i] = (n + 3) * U53 * (sf + g) + g + U53 * np.abs(h[i])
            e_cell = np.where(owned, hbound[i][region], 0.0)
            hv = self.bcast(h[i]) * self.planes(v)
            dev = np.where(owned, dev + e_cell * np.abs(v) + U53 * (1 + U53) * (
                2 * np.abs(w) + dev + 4 * np.abs(hv.reshape(-1)) + 2 * e_cell * np.abs(v)), 0.0)
            w = (self.planes(w) - hv).reshape(-1)
        return h, w, hbound
