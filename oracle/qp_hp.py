"""ORACLE -- test infrastructure (see oracle/__init__.py): one QP of the SQP loop in extended precision.

The formulas of oracle/sqp.py (schur_blocks, recover_dxu, the BJ / SS preconditioner's diagonal blocks) with
every array and scalar in np.longdouble (the x87 80-bit format, eps 1.1e-19; backward_hp of oracle/ilqr.py
relies on the same).  np.linalg has no long-double path, so the eliminations are written out; `@` on
long-double arrays runs numpy's own loops.  The kernels' fp64 results and the fp64 oracle's are both compared
against these, so an error is measured, not a difference between two roundings.
"""
import numpy as np

HP = np.longdouble


def hp(a):
    return np.asarray(a, dtype=HP)


def inv_hp(M):
    """M^-1 by Gauss-Jordan with partial pivoting."""
    M = hp(M)
    n = M.shape[0]
    a = np.concatenate([M.copy(), np.eye(n, dtype=HP)], axis=1)
    for p in range(n):
        r = p + int(np.argmax(np.abs(a[p:, p])))
        if a[r, p] == 0:
            raise np.linalg.LinAlgError("singular matrix")
        if r != p:
            a[[p, r]] = a[[r, p]]
        a[p] = a[p] / a[p, p]
        f = a[:, p].copy()
        f[p] = 0
        a -= np.outer(f, a[p])
    return a[:, n:]


def _solve_hp(M, rhs):
    """M^-1 rhs (rhs a vector or a matrix) by Gaussian elimination with partial pivoting"""
    M, rhs = hp(M), hp(rhs)
    n = M.shape[0]
    vec = rhs.ndim == 1
    a = np.concatenate([M.copy(), rhs.reshape(n, -1).copy()], axis=1)
    for p in range(n):
        r = p + int(np.argmax(np.abs(a[p:, p])))
        if a[r, p] == 0:
            raise np.linalg.LinAlgError("singular matrix")
        if r != p:
            a[[p, r]] = a[[r, p]]
        f = a[p + 1:, p] / a[p, p]
        a[p + 1:] -= np.outer(f, a[p])
    x = np.zeros((n, a.shape[1] - n), dtype=HP)
    for p in range(n - 1, -1, -1):
        x[p] = (a[p, n:] - a[p, p + 1:n] @ x[p + 1:]) / a[p, p]
    return x[:, 0] if vec else x


def ghat_hp(G, rho):
    """inv_hp(G_k + rho I) per knot"""
    rho = HP(rho)
    return [inv_hp(hp(Gk) + rho * np.eye(len(Gk), dtype=HP)) for Gk in G]


def schur_hp(G, g, A, B, c, rho, nx, Gh=None):
    """schur_blocks of oracle/sqp.py: G, g the per-knot cost blocks (lists; the terminal knot's nx wide), A, B
    [N-1], c [N][nx] -> Gh (list), Sd [N][nx][nx], Sl [N-1][nx][nx] (S_{k+1,k}), gam [N][nx].  Gh: ghat_hp(G, rho)
    when the caller already has it."""
    N = len(G)
    if Gh is None:
        Gh = ghat_hp(G, rho)
    g = [hp(gk) for gk in g]
    A, B, c = hp(A), hp(B), hp(c)
    Sd = np.zeros((N, nx, nx), dtype=HP)
    Sl = np.zeros((N - 1, nx, nx), dtype=HP)
    gam = np.zeros((N, nx), dtype=HP)
    Sd[0] = -Gh[0][:nx, :nx]
    gam[0] = c[0] - (Gh[0] @ g[0])[:nx]
    for k in range(N - 1):
        AB = np.hstack((A[k], B[k]))
        ABG = AB @ Gh[k]
        Sd[k + 1] = -(ABG @ AB.T + Gh[k + 1][:nx, :nx])
        Sl[k] = ABG[:, :nx]
        gam[k + 1] = c[k + 1] + ABG @ g[k] - (Gh[k + 1] @ g[k + 1])[:nx]
    return Gh, Sd, Sl, gam


def solve_hp(Sd, Sl, gam):
    """lambda of S lambda = gamma for the symmetric block-tridiagonal S (diagonal blocks Sd, sub-diagonal blocks
    Sl = S_{k+1,k}, super-diagonal their transposes) by block elimination, O(N nx^3): [N][nx]."""
    Sd, Sl, gam = hp(Sd), hp(Sl), hp(gam)
    N, nx, _ = Sd.shape
    gam = gam.reshape(N, nx)
    D = [Sd[0]]
    y = [gam[0]]
    W = []   # W_k = D_k^-1 S_{k,k+1}
    for k in range(N - 1):
        sol = _solve_hp(D[k], np.concatenate([Sl[k].T, y[k][:, None]], axis=1))
        W.append(sol[:, :nx])
        D.append(Sd[k + 1] - Sl[k] @ sol[:, :nx])
        y.append(gam[k + 1] - Sl[k] @ sol[:, nx])
    lam = np.zeros((N, nx), dtype=HP)
    lam[N - 1] = _solve_hp(D[N - 1], y[N - 1])
    for k in range(N - 2, -1, -1):
        lam[k] = _solve_hp(D[k], y[k]) - W[k] @ lam[k + 1]
    return lam


def residual_hp(Sd, Sl, gam, lam):
    """S lam - gamma [N][nx] for the block-tridiagonal S"""
    Sd, Sl, lam = hp(Sd), hp(Sl), hp(lam)
    N, nx, _ = Sd.shape
    L = lam.reshape(N, nx)
    r = np.einsum("kij,kj->ki", Sd, L) - hp(gam).reshape(N, nx)
    if N > 1:
        r[1:] += np.einsum("kij,kj->ki", Sl, L[:-1])
        r[:-1] += np.einsum("kji,kj->ki", Sl, L[1:])
    return r


def backward_error(Sd, Sl, gam, lam):
    """the normwise backward error |S lam - gamma|_inf / (|S|_inf |lam|_inf + |gamma|_inf) in long double"""
    Sd, Sl = hp(Sd), hp(Sl)
    N, nx, _ = Sd.shape
    rows = np.sum(np.abs(Sd), axis=2)
    if N > 1:
        rows[1:] += np.sum(np.abs(Sl), axis=2)
        rows[:-1] += np.sum(np.abs(Sl), axis=1)
    r = residual_hp(Sd, Sl, gam, lam)
    return float(np.max(np.abs(r)) / (np.max(rows) * np.max(np.abs(hp(lam))) + np.max(np.abs(hp(gam)))))


def dxu_hp(Gh, g, A, B, lam, nx):
    """recover_dxu of oracle/sqp.py without the lambda tail: the knots' [dx_k; du_k] concatenated"""
    N = len(Gh)
    A, B = hp(A), hp(B)
    L = hp(lam).reshape(N, nx)
    out = []
    for k in range(N - 1):
        ctl = np.concatenate([L[k] - A[k].T @ L[k + 1], -B[k].T @ L[k + 1]])
        out.append(hp(Gh[k]) @ (hp(g[k]) - ctl))
    out.append(hp(Gh[N - 1]) @ (hp(g[N - 1]) - L[N - 1]))
    return np.concatenate(out)


def precond_diag_hp(Sd):
    """the BJ / SS preconditioner's diagonal blocks S_kk^-1 [N][nx][nx]"""
    return np.array([inv_hp(S) for S in hp(Sd)])
