"""The Riemannian staircase over the multi-agent RBCD engine (SE-Sync / DC2-PGO; the reference has none).

At each rank r the engine runs its colour schedule to a critical point, the whole-graph certificate
(Graph.certify) decides whether it is the global optimum of the relaxation, and if not Graph.escape moves off the
saddle [X; 0] of the rank r + 1 problem along the certificate's negative-curvature direction; the next engine starts
there.  With reduce_tol the certified solution is then truncated to its numerical rank (Graph.rank_reduce) and
certified again there.  One rank (world = 1) only: every agent lives in this process."""
from __future__ import annotations

import numpy as np

from . import hip as H


class StaircaseError(RuntimeError):
    pass


def solve(graph: "H.Graph", agent_of_pose, agent_rank, X0, r0, params: "H.RbcdParams | None" = None, r_max=8,
          eta=1e-6, grad_tol=1e-6, max_steps=10000, cert=None, escape=None, reduce_tol=None, certifier="lanczos"):
    """Solve the pose graph from X0 (r0 x (d+1) n matrix, or its flat column-major buffer), raising the rank until
    the certificate holds.

    Per level: an Rbcd at rank r (params with r replaced) from set_X; colour-schedule steps until central_eval's
    total |RieGrad| < grad_tol or max_steps; get_X_into; Graph.certify(want_vector=True, **cert).  lambda_min >= -eta
    ends the staircase; otherwise Graph.escape (escape: EscapeParams fields; min_gradnorm defaults to the engine's
    tolerance, below which an agent's solve returns its input) starts rank r + 1.

    Returns (X flat r x (d+1) n column-major, r, levels) with one dict(r, steps, f, gradnorm, lambda_min, alpha,
    trials) per level (alpha = trials = 0 on the last).  Raises StaircaseError when r_max is reached uncertified or an
    escape is not accepted.  Single rank only (world = 1): agent_rank must be all zero.

    reduce_tol (None: nothing more happens): after certification at rank r, Graph.rank_reduce(X, r, reduce_tol)
    truncates X to its numerical rank k; when k < r an engine at rank k runs from the reduced X (0 or more steps, until
    grad_tol or max_steps) and Graph.certify decides at rank k.  The rank-k X is returned when it certifies
    (lambda_min >= -eta), the certified rank-r X otherwise; either way levels gains one entry for rank k that also
    carries reduced_from = r, dropped (the Gram eigenvalues cut off), w (the Gram's spectrum) and certified.  When
    the numerical rank is r itself nothing is added and the return is that of reduce_tol=None.

    certifier="chol": every certificate is Graph.certify_chol(X, r, eta) instead (the Cholesky test of S(X) + eta I,
    and on failure a bracket and inverse iteration for lambda_min and its vector); `cert` then holds
    dpgo_chol_cert_params fields.  A certified level records lambda_min = -eta (the bound the test proves) and
    pd = True, an uncertified one pd = False; each carries factorisations and invit_iters.  A level whose whole-graph
    factor is refused for its size is certified by Graph.certify with its defaults and records fallback = True.

    certifier="lobpcg": every certificate is Graph.certify_block(X, r) (LOBPCG on the r lifted rows, any graph size);
    `cert` then holds dpgo_block_cert_params fields.  A level is certified when the certificate's lower_bound >= -eta
    (the bound, not the Ritz value, which only bounds lambda_min from above) and records lower_bound, bound_ok and
    iters (operator passes); an uncertified level escapes along the certificate's vector.  A level whose bound fails
    while its lambda_min is not negative (an unconverged certificate) raises StaircaseError."""
    if certifier not in ("lanczos", "chol", "lobpcg"):
        raise StaircaseError(f"unknown certifier {certifier!r}")
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

    def run_level(r, X):
        """One engine at rank r from X to a critical point: (X, steps, f, gradnorm)."""
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
        return X, steps, f, float(np.sqrt(gsq.sum())), p

    def certify(X, r):
        """The level's certificate: (dict with lambda_min and, when it is negative, eigvec; extra level fields)."""
        if certifier == "lanczos":
            return graph.certify(X, r, want_vector=True, **cert), {}
        if certifier == "lobpcg":
            c = graph.certify_block(X, r, **cert)
            return c, dict(lower_bound=c["lower_bound"], bound_ok=bool(c["lower_bound"] >= -eta), iters=c["iters"])
        try:
            c = graph.certify_chol(X, r, eta, **cert)
        except H.DPGOHipError as e:
            if "GiB" not in str(e) and "memory" not in str(e).lower():
                raise
            return graph.certify(X, r, want_vector=True), dict(fallback=True)
        return c, dict(pd=c["pd"], fallback=False, factorisations=c["factorisations"], invit_iters=c["invit_iters"])

    while True:
        X, steps, f, gradnorm, p = run_level(r, X)
        c, extra = certify(X, r)
        lam = c["lambda_min"]
        levels.append(dict(r=r, steps=steps, f=f, gradnorm=gradnorm, lambda_min=lam, alpha=0.0, trials=0, **extra))
        if extra.get("pd", extra.get("bound_ok", lam >= -eta)):  # the certifier's own decision where it made one
            break
        if not lam < 0.0:
            raise StaircaseError(f"rank {r} undecided: lower_bound = {extra.get('lower_bound')}, lambda_min = {lam:.3e}")
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
    if reduce_tol is None:
        return X, r, levels
    k, Xk, info = graph.rank_reduce(X, r, reduce_tol)
    if k == r:
        return X, r, levels
    Xk, steps, f, gradnorm, _ = run_level(k, Xk)
    c, extra = (graph.certify(Xk, k, **cert), {}) if certifier == "lanczos" else certify(Xk, k)
    lam = c["lambda_min"]
    levels.append(dict(r=k, steps=steps, f=f, gradnorm=gradnorm, lambda_min=lam, alpha=0.0, trials=0, reduced_from=r,
                       dropped=info["dropped"], w=info["w"],
                       certified=bool(extra.get("pd", extra.get("bound_ok", lam >= -eta))), **extra))
    return (Xk, k, levels) if levels[-1]["certified"] else (X, r, levels)
