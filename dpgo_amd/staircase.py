"""The Riemannian staircase over the multi-agent RBCD engine (SE-Sync / DC2-PGO; the reference has none).

At each rank r the engine runs its colour schedule to a critical point, the whole-graph certificate
(Graph.certify) decides whether it is the global optimum of the relaxation, and if not Graph.escape moves off the
saddle [X; 0] of the rank r + 1 problem along the certificate's negative-curvature direction; the next engine starts
there.  One rank (world = 1) only: every agent lives in this process."""
from __future__ import annotations

import numpy as np

from . import hip as H


class StaircaseError(RuntimeError):
    pass


def solve(graph: "H.Graph", agent_of_pose, agent_rank, X0, r0, params: "H.RbcdParams | None" = None, r_max=8,
          eta=1e-6, grad_tol=1e-6, max_steps=10000, cert=None, escape=None):
    """Solve the pose graph from X0 (r0 x (d+1) n matrix, or its flat column-major buffer), raising the rank until
    the certificate holds.

    Per level: an Rbcd at rank r (params with r replaced) from set_X; colour-schedule steps until central_eval's
    total |RieGrad| < grad_tol or max_steps; get_X_into; Graph.certify(want_vector=True, **cert).  lambda_min >= -eta
    ends the staircase; otherwise Graph.escape (escape: EscapeParams fields; min_gradnorm defaults to the engine's
    tolerance, below which an agent's solve returns its input) starts rank r + 1.

    Returns (X flat r x (d+1) n column-major, r, levels) with one dict(r, steps, f, gradnorm, lambda_min, alpha,
    trials) per level (alpha = trials = 0 on the last).  Raises StaircaseError when r_max is reached uncertified or an
    escape is not accepted.  Single rank only (world = 1): agent_rank must be all zero."""
    ar = np.asarray(agent_rank, dtype=np.int32)
    if np.any(ar != 0):
        raise StaircaseError("staircase.solve runs on one rank: agent_rank must be all zero")
    base = params or H.rbcd_params()
    cert = dict(cert or {})
    X0 = np.asarray(X0, dtype=np.float64)
    X = H.to_dev_layout(X0) if X0.ndim == 2 else np.ascontiguousarray(X0).ravel()
    bn = (graph.d + 1) * graph.n
    if X.size != r0 * bn:
        raise StaircaseError("X0 has the wrong size for r0")
    r, levels = int(r0), []
    while True:
        p = H.RbcdParams()
        for k, _ in H.RbcdParams._fields_:
            setattr(p, k, getattr(base, k))
        p.r = r
        e = H.Rbcd(graph, agent_of_pose, ar, 0, 1, p)
        try:
            e.set_X(X)
            steps = 0
            f, gsq = e.central_eval()
            while float(np.sqrt(gsq.sum())) >= grad_tol and steps < max_steps:
                c = steps % e.num_colors
                e.pre_exchange(c)
                e.update(c, None)
                steps += 1
                f, gsq = e.central_eval()
            X = np.zeros(r * bn)
            e.get_X_into(X)
        finally:
            e.close()
        c = graph.certify(X, r, want_vector=True, **cert)
        lam = c["lambda_min"]
        levels.append(dict(r=r, steps=steps, f=f, gradnorm=float(np.sqrt(gsq.sum())), lambda_min=lam, alpha=0.0,
                           trials=0))
        if lam >= -eta:
            return X, r, levels
        if r >= r_max:
            raise StaircaseError(f"rank {r} reached uncertified: lambda_min = {lam:.3e}")
        ep = H.escape_params(min_gradnorm=p.tolerance)
        for k, v in (escape or {}).items():
            setattr(ep, k, v)
        X, info = graph.escape(X, r, c["eigvec"], lam, ep)
        levels[-1].update(alpha=info["alpha"], trials=info["trials"])
        if not info["accepted"]:
            raise StaircaseError(f"escape from rank {r} not accepted: {info}")
        r += 1
