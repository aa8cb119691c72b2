"""Extended-precision (np.longdouble, 64-bit mantissa) restatement of one ROPTLIB RTR Run: the reference trajectory the
float64 implementations -- oracle and device -- are measured against.  Test infrastructure."""
import numpy as np


def gauss_jordan_inverse(M):
    """M^-1 of one square block by Gauss-Jordan with partial pivoting in np.longdouble."""
    L = np.longdouble
    b = M.shape[0]
    A = np.concatenate([np.asarray(M, dtype=L), np.eye(b, dtype=L)], axis=1)
    for c in range(b):
        piv = c + int(np.argmax(np.abs(A[c:, c])))
        A[[c, piv]] = A[[piv, c]]
        A[c] /= A[c, c]
        for u in range(b):
            if u != c:
                A[u] -= A[u, c] * A[c]
    return A[:, b:]


def rtr_extended(Q, X0, d, tol, Delta0, Delta_max, max_iter, max_inner, precon="bj", return_state=False):
    """ROPTLIB RTR Run (A.4: tCG from eta = 0, QF retraction, rho test, radius update; G = 0) in extended precision
    (np.longdouble, 64-bit mantissa): the record sequence of _expected_records, as the reference trajectory the
    float64 implementations are measured against.  Q is applied as a sparse product in extended precision.
    precon "bj": per-pose (Q_jj + 0.1 I)^-1 by Gauss-Jordan in extended precision; "exact": (Q + 0.1 I)^-1
    (src/QuadraticProblem.cpp:31-42, 75-87) by a float64 sparse LU refined in extended precision until the residual
    is at the extended rounding level (each refinement step gains ~ -log10(cond * eps64) digits).
    return_state: (records, x, f(x), accepted) with x the Run's last accepted iterate in extended precision."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    L = np.longdouble
    r = X0.shape[0]
    b = d + 1
    n = X0.shape[1] // b
    # an explicit (possibly zero) diagonal: a pose without measurements has an empty row otherwise
    Qo = sp.coo_matrix(Q)
    dg = np.arange(Qo.shape[0])
    Qc = sp.csr_matrix((np.concatenate([Qo.data, np.zeros(len(dg))]),
                        (np.concatenate([Qo.row, dg]), np.concatenate([Qo.col, dg]))), shape=Qo.shape)
    Qc.sum_duplicates()
    Qc.sort_indices()
    q_val, q_idx, q_ptr = Qc.data.astype(L), Qc.indices, Qc.indptr
    assert np.all(np.diff(q_ptr) > 0)  # reduceat needs no empty row

    def qmul(V):  # (Q V^T)^T, r x N, every product and sum in extended precision
        return np.add.reduceat(V[:, q_idx] * q_val[None, :], q_ptr[:-1], axis=1)
    P = lambda V: V.reshape(r, n, b).transpose(1, 0, 2)  # noqa: E731  pose blocks (n, r, b)
    U = lambda Pb: Pb.transpose(1, 0, 2).reshape(r, n * b)  # noqa: E731
    ip = lambda A_, B_: np.sum(A_ * B_, dtype=L)  # noqa: E731
    sym = lambda M: 0.5 * (M + np.swapaxes(M, 1, 2))  # noqa: E731
    if precon == "exact":
        lu = spla.splu((Qc + 0.1 * sp.identity(Qc.shape[0], format="csr")).tocsc())

        def psolve(V):  # V (Q + 0.1 I)^-1 with iterative refinement in extended precision
            Z = lu.solve(np.ascontiguousarray(V.astype(np.float64).T)).T.astype(L)
            for _ in range(6):
                Res = V - (qmul(Z) + L(0.1) * Z)
                if np.max(np.abs(Res)) <= L(1e-19) * max(np.max(np.abs(V)), L(1e-300)):
                    break
                Z = Z + lu.solve(np.ascontiguousarray(Res.astype(np.float64).T)).T.astype(L)
            return Z
    else:
        Minv = np.zeros((n, b, b), L)  # (Q_jj + 0.1 I)^-1 by Gauss-Jordan in extended precision
        for j in range(n):
            Minv[j] = gauss_jordan_inverse(Qc[j * b:(j + 1) * b, j * b:(j + 1) * b].toarray().astype(L) +
                                           L(0.1) * np.eye(b, dtype=L))
        psolve = lambda V: U(P(V) @ Minv)  # noqa: E731

    def proj(X, V):
        Y = P(X)[:, :, :d]
        Vp = P(V).copy()
        VY = Vp[:, :, :d]
        Vp[:, :, :d] = VY - Y @ sym(np.swapaxes(Y, 1, 2) @ VY)
        return U(Vp)

    def retract(X, V):  # [qf(Y + V_Y) | p + V_p], qf by modified Gram-Schmidt (positive diagonal)
        Pp = P(X + V).copy()
        for j in range(n):
            M = Pp[j, :, :d]
            for c in range(d):
                v = M[:, c].copy()
                for k in range(c):
                    v = v - np.sum(M[:, k] * v, dtype=L) * M[:, k]
                M[:, c] = v / np.sqrt(np.sum(v * v, dtype=L))
            Pp[j, :, :d] = M
        return U(Pp)

    egrad = qmul
    fval = lambda X: L(0.5) * ip(egrad(X), X)  # noqa: E731
    x1 = X0.astype(L)
    EG = egrad(x1)
    f1 = fval(x1)
    g = proj(x1, EG)
    ngf = np.sqrt(ip(g, g))
    Delta, it, recs = L(Delta0), 0, []
    accepted = False
    while not (ngf < tol) and it < max_iter:
        S = sym(np.swapaxes(P(x1)[:, :, :d], 1, 2) @ P(EG)[:, :, :d])

        def hess(V):
            H_ = P(egrad(V)).copy()
            H_[:, :, :d] -= P(V)[:, :, :d] @ S
            return proj(x1, U(H_))

        prec = lambda V: proj(x1, psolve(V))  # noqa: E731
        eta = np.zeros_like(x1)
        Heta = np.zeros_like(x1)
        rv = g.copy()
        z = prec(rv)
        z_r = ip(z, rv)
        d_Pd, e_Pe, e_Pd = z_r, L(0), L(0)
        delta = -z
        norm_r0 = np.sqrt(ip(rv, rv))
        status, ninner = 4, max_inner
        for j in range(max_inner):
            Hd = hess(delta)
            d_Hd = ip(delta, Hd)
            alpha = z_r / d_Hd
            e_Pe_new = e_Pe + 2 * alpha * e_Pd + alpha * alpha * d_Pd
            rec = dict(op=3, j=j, d_Hd=d_Hd, alpha=alpha, Delta=Delta)
            if d_Hd <= 0 or e_Pe_new >= Delta * Delta:
                tau = (-e_Pd + np.sqrt(e_Pd * e_Pd + d_Pd * (Delta * Delta - e_Pe))) / d_Pd
                eta = eta + tau * delta
                Heta = Heta + tau * Hd
                status = 0 if d_Hd <= 0 else 1
                rec.update(tau=tau, status=status)
                recs.append(rec)
                ninner = j + 1
                break
            recs.append(rec)
            e_Pe = e_Pe_new
            eta = eta + alpha * delta
            Heta = Heta + alpha * Hd
            rv = rv + alpha * Hd
            norm_r = np.sqrt(ip(rv, rv))
            if norm_r <= norm_r0 * min(norm_r0, L(0.1)):
                status = 2 if L(0.1) < norm_r0 else 3
                recs.append(dict(op=4, j=j, norm_r=norm_r, status=status))
                ninner = j + 1
                break
            zn = prec(rv)
            zr_new = ip(zn, rv)
            beta = zr_new / z_r
            recs.append(dict(op=4, j=j, norm_r=norm_r, z_r=zr_new, beta=beta))
            z_r = zr_new
            delta = -zn + beta * delta
            e_Pd = beta * (e_Pd + alpha * d_Pd)
            d_Pd = z_r + beta * beta * d_Pd
        x2 = retract(x1, eta)
        f2 = fval(x2)
        rho = (f1 - f2) / (-ip(g, eta) - L(0.5) * ip(eta, Heta))
        accepted = rho > L(0.1)
        recs.append(dict(op=5, f1=f1, f2=f2, rho=rho, Delta=Delta, accepted=float(accepted), ngf=ngf, status=status,
                         alpha=ninner))
        if rho < L(0.25):
            Delta = L(0.25) * Delta
        elif rho > L(0.75) and status in (0, 1):
            Delta = min(2 * Delta, L(Delta_max))
        if accepted:
            x1, f1 = x2, f2
            EG = egrad(x1)
            g = proj(x1, EG)
            ngf = np.sqrt(ip(g, g))
        it += 1
    recs = [{k: (float(v) if isinstance(v, np.floating) else v) for k, v in rec.items()} for rec in recs]
    return (recs, x1, f1, bool(accepted)) if return_state else recs


def optimize_extended(Q, X0, d, tol, radius, max_inner, precon="bj"):
    """QuadraticOptimizer::trustRegion with tr_iterations = 1 (src/QuadraticOptimizer.cpp:92-110) over rtr_extended:
    single-iteration Runs, the radius quartered after a rejected step, at most 12 of them.  (x, f(x), runs), x the
    accepted iterate (X0 when every Run was rejected), in extended precision."""
    runs, steps = 0, 0
    while True:
        recs, x, f, acc = rtr_extended(Q, X0, d, tol, radius, radius, 1, max_inner, precon, return_state=True)
        runs += 1
        if acc or steps > 10 or not recs:
            return x, f, runs
        radius /= 4.0
        steps += 1
