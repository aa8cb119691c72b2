"""The noise-free ring pose graphs on which the rank-r relaxation has a strict local minimum that is not global, and
a numpy restatement of the rank staircase (test infrastructure).

Ring: n = 12 poses, edges j -> (j + 1) mod 12, every measurement R~ = Rot(2 pi / 12) (about z for d = 3),
t~ = e_1, kappa = tau = 1: f* = 0 at the winding-1 circle.  The winding-2 configuration Y_j = Rot(j 4 pi / 12)
(translations fitted) is a second-order critical point of the rank-d problem with f = 24 (1 - cos 30 deg) and
lambda_min(S) = -0.1304 (a double eigenvalue).

The escape, its line search and the staircase are restated from the oracle's retract_qf, certificate_matrix and
rtr_run / Agent: X+(alpha) = Retr_[X; 0](alpha [0; v^T]), backtracking on alpha until
f(X+) <= f([X; 0]) + decrease alpha^2 lambda_min."""
import math

import numpy as np

from oracle import dpgo_oracle as O

N_RING = 12
F_CRIT = 24.0 * (1.0 - math.cos(math.pi / 6.0))


def _rot(d, theta):
    R = np.eye(d)
    c, s = math.cos(theta), math.sin(theta)
    R[0, 0], R[0, 1], R[1, 0], R[1, 1] = c, -s, s, c
    return R


def ring(d, n=N_RING):
    """The ring's measurements (oracle Measurements, one robot)."""
    p1 = np.arange(n, dtype=np.int64)
    p2 = (p1 + 1) % n
    R = np.repeat(_rot(d, 2.0 * math.pi / n)[None], n, axis=0)
    t = np.zeros((n, d))
    t[:, 0] = 1.0
    z = np.zeros(n, np.int64)
    return O.Measurements(d, z, z.copy(), p1, p2, R, t, np.ones(n), np.ones(n), np.ones(n), n)


def winding2(meas):
    """Y_j = Rot(j 4 pi / n) at r = d with the least-squares translations: d x (d+1) n."""
    d, n = meas.d, meas.num_poses
    b = d + 1
    Q = O.connection_laplacian(meas, n).toarray()
    X = np.zeros((d, b * n))
    rot = np.concatenate([np.arange(j * b, j * b + d) for j in range(n)])
    tra = np.arange(d, b * n, b)
    for j in range(n):
        X[:, j * b:j * b + d] = _rot(d, j * 4.0 * math.pi / n)
    # f is quadratic in the translations: Q_pp p^T = -Q_pY Y^T (Q_pp a graph Laplacian: minimum-norm solution)
    X[:, tra] = -np.linalg.lstsq(Q[np.ix_(tra, tra)], Q[np.ix_(tra, rot)] @ X[:, rot].T, rcond=None)[0].T
    return X


def cost(Q, X):
    return 0.5 * float(np.sum(np.asarray((Q @ X.T).T) * X))


def gradnorm(Q, X, d):
    return float(np.linalg.norm(O.tangent_project(X, np.asarray((Q @ X.T).T), d)))


def min_eig(Q, X, d):
    """(lambda_min, unit eigenvector) of the certificate matrix S(X), dense."""
    w, V = np.linalg.eigh(O.certificate_matrix(Q, X, d).toarray())
    return float(w[0]), V[:, 0].copy()


def lift(X):
    return np.vstack([X, np.zeros((1, X.shape[1]))])


def escape_point(X, v, alpha, d):
    """Retr_[X; 0](alpha [0; v^T]) with the oracle's QF retraction: (r + 1) x (d+1) n."""
    D = np.zeros((X.shape[0] + 1, X.shape[1]))
    D[-1] = alpha * np.asarray(v)
    return O.retract_qf(lift(X), D, d)


def escape_direction(vec):
    """The row of largest 2-norm of a Ritz matrix (every non-zero row is an eigenvector of S), normalised."""
    V = np.atleast_2d(np.asarray(vec, dtype=float))
    row = V[int(np.argmax(np.linalg.norm(V, axis=1)))]
    return row / np.linalg.norm(row)


def line_search(Q, X, v, lam, d, alpha0=1.0, decrease=0.25, min_gradnorm=0.0, max_halvings=30):
    """The escape's backtracking: (X_out, info) with info = dict(accepted, trials, alpha, f_before, f_after,
    gradnorm_after).  Not accepted (no alpha passed, or |RieGrad(X+)| < min_gradnorm): X_out = [X; 0]."""
    f0 = cost(Q, lift(X))
    info = dict(accepted=0, trials=0, alpha=0.0, f_before=f0, f_after=f0, gradnorm_after=0.0)
    for k in range(max_halvings + 1):
        alpha = alpha0 * 2.0 ** -k
        Xp = escape_point(X, v, alpha, d)
        fp = cost(Q, Xp)
        info.update(trials=k + 1, alpha=alpha, f_after=fp)
        if fp <= f0 + decrease * alpha * alpha * lam:
            info["gradnorm_after"] = gradnorm(Q, Xp, d)
            if info["gradnorm_after"] >= min_gradnorm:
                info["accepted"] = 1
                return Xp, info
            break
    return lift(X), info


def staircase_rtr(meas, X0, r_max=8, tol=1e-9, eta=1e-9):
    """The staircase with the oracle's RTR at every level: (X, [dict(r, f, gradnorm, lambda_min, alpha, trials)])."""
    d, n = meas.d, meas.num_poses
    Q = O.connection_laplacian(meas, n)
    X, levels = X0.copy(), []
    while True:
        r = X.shape[0]
        P = O.QuadraticProblem(n, d, r)
        P.set_Q(Q)
        X, _, _, info = O.rtr_run(P, X, tol, 10.0, 1e3, 500, 200)
        lam, v = min_eig(Q, X, d)
        levels.append(dict(r=r, f=info["f"], gradnorm=info["ngf"], lambda_min=lam, alpha=0.0, trials=0))
        if lam >= -eta or r >= r_max:
            return X, levels
        X, esc = line_search(Q, X, v, lam, d, min_gradnorm=tol)
        assert esc["accepted"] == 1, esc
        levels[-1].update(alpha=esc["alpha"], trials=esc["trials"])


class _Agent(O.Agent):
    """The oracle's PGOAgent restatement with the engine's `tolerance` parameter (the oracle fixes it at the
    reference's 1e-2)."""
    tolerance = 1e-2

    def update_X(self, do_opt, accel, trace=None):
        if not do_opt:
            return super().update_X(do_opt, accel, trace)
        ok = self.construct_G(self.neighbor_aux_pose if accel else self.neighbor_pose)
        if not ok:
            return False
        params = O.OptParams(algorithm=self.p.algorithm, tr_iterations=1, tr_tolerance=self.tolerance,
                             tr_initial_radius=100.0, tr_max_inner=10)
        self.X, self.last_result = O.optimize(self.problem, self.Y if accel else self.X, params, trace)
        return True


def rbcd_level(meas, agent_of_pose, num_agents, X0, accel, tolerance, grad_tol, max_steps):
    """O.colour_rbcd's schedule (L2, block-Jacobi), stepped until the central |RieGrad| < grad_tol or max_steps:
    (X, steps, f, gradnorm)."""
    d, n, r = meas.d, len(agent_of_pose), X0.shape[0]
    b = d + 1
    Q = O.connection_laplacian(meas, n)
    aop = np.asarray(agent_of_pose)
    local, counts = np.zeros(n, np.int64), np.zeros(num_agents, np.int64)
    for i in range(n):
        local[i] = counts[aop[i]]
        counts[aop[i]] += 1
    parts = O._split(meas, aop, local, num_agents)
    cols = [np.concatenate([np.arange(p * b, (p + 1) * b) for p in np.nonzero(aop == a)[0]])
            for a in range(num_agents)]
    agents = []
    for a in range(num_agents):
        ag = _Agent(a, O.AgentParams(d, r, num_agents, acceleration=accel, robust="L2",
                                     precon=O.PRECON_BLOCK_JACOBI))
        ag.tolerance = tolerance
        ag.set_pose_graph(*parts[a], n=int(counts[a]))
        ag.set_X(X0[:, cols[a]])
        agents.append(ag)
    colors = O.greedy_colors(meas, aop, num_agents)
    C = max(colors) + 1

    def gather():
        X = np.zeros_like(X0)
        for a, ag in enumerate(agents):
            X[:, cols[a]] = ag.X
        return X

    X, steps = X0.copy(), 0
    while gradnorm(Q, X, d) >= grad_tol and steps < max_steps:
        c = steps % C
        for ag in agents:
            if colors[ag.id] != c:
                ag.iterate(False)
        for ag in agents:
            if colors[ag.id] != c:
                continue
            for other in agents:
                if other.id == ag.id:
                    continue
                ag.update_neighbor_poses(other.id, other.shared_pose_dict(False), aux=False)
                if accel:
                    ag.update_neighbor_poses(other.id, other.shared_pose_dict(True), aux=True)
        for ag in agents:
            if colors[ag.id] == c:
                ag.iterate(True)
        steps += 1
        X = gather()
    return X, steps, cost(Q, X), gradnorm(Q, X, d)


def staircase_rbcd(meas, agent_of_pose, num_agents, X0, accel, tolerance=1e-9, grad_tol=1e-7, eta=1e-6,
                   max_steps=20000, r_max=8):
    """dpgo_amd.staircase.solve replayed on the CPU: rbcd_level per rank, the dense certificate, the numpy
    escape.  Returns (X, levels) with levels as staircase_rtr's plus `steps`."""
    d, n = meas.d, meas.num_poses
    Q = O.connection_laplacian(meas, n)
    X, levels = X0.copy(), []
    while True:
        r = X.shape[0]
        X, steps, f, gn = rbcd_level(meas, agent_of_pose, num_agents, X, accel, tolerance, grad_tol, max_steps)
        lam, v = min_eig(Q, X, d)
        levels.append(dict(r=r, steps=steps, f=f, gradnorm=gn, lambda_min=lam, alpha=0.0, trials=0))
        if lam >= -eta or r >= r_max:
            return X, levels
        X, esc = line_search(Q, X, v, lam, d, min_gradnorm=tolerance)
        assert esc["accepted"] == 1, esc
        levels[-1].update(alpha=esc["alpha"], trials=esc["trials"])
