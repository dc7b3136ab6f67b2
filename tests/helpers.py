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
