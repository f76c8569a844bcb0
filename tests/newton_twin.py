"""NumPy twin of the tangent-space CG of Newton's method (csrc/newton_kernels.hip, dftk_jl_amd/newton.py), written from the
algorithm: the preconditioned conjugate gradients with a projection after every update and a custom inner product, for one
right-hand side, on "packed vectors" -- lists of complex blocks, one per k-point, with a weight each.

* ``wdot``: the inner product sum_b w_b Re <a_b, b_b>.
* ``cg``: the recursion in one piece.
* ``CgScalars``: the same recursion cut into the pieces the C ABI has (``dot`` into a named slot, ``update_xr`` forming alpha
  from the slots, ``update_p`` forming beta, ``read``), so that a device run can be followed call by call.

``real`` is the working precision: ``numpy.longdouble`` (the reference of the device tests) or ``numpy.float64`` (the same
formulas in the device's precision: its distance from the longdouble run is what the tests' bounds are made of).
"""
import numpy as np

LD = np.longdouble
GAMMA, PC, RR = 0, 1, 2


def ctype(real):
    return np.clongdouble if real is LD else np.complex128


def cast(blocks, real=LD):
    return [np.asarray(b).astype(ctype(real)) for b in blocks]


def wdot(a, b, w, real=LD):
    """sum_b w_b Re <a_b, b_b>, every block summed for itself, the blocks in order"""
    tot = real(0)
    for x, y, wb in zip(a, b, w):
        x, y = np.asarray(x).astype(ctype(real)), np.asarray(y).astype(ctype(real))
        tot = tot + real(wb) * np.sum(x.real * y.real + x.imag * y.imag, dtype=real)
    return tot


def cg(apply_A, b, weights, precon=None, proj=None, tol=1e-10, maxiter=100, miniter=1, real=LD):
    """x with A x = b from x = 0.  ``apply_A``, ``precon`` and ``proj`` map packed vectors to packed vectors (``precon``
    applies the inverse of the preconditioner).  The order of operations per iteration: c = A p; alpha = gamma / <p, c>;
    x = proj(x + alpha p); r = proj(r - alpha c); the residual norm sqrt(<r, r>); c = precon(r); gamma' = <r, c>;
    beta = gamma' / gamma; p = proj(c + beta p).  Convergence (residual norm <= tol, at least ``miniter`` iterations begun) is
    tested at the head of an iteration.  ``<p, A p> <= 0`` ends the run with ``negative_curvature``.  Returns a dict."""
    precon = precon or (lambda v: [u.copy() for u in v])
    proj = proj or (lambda v: v)
    r = cast(b, real)
    x = [np.zeros_like(u) for u in r]
    c = cast(precon(r), real)
    gamma = wdot(r, c, weights, real)
    p = [u.copy() for u in c]
    history = [np.sqrt(wdot(r, r, weights, real))]
    n_iter, converged, negative = 0, False, False
    alphas, betas = [], []
    while n_iter < maxiter:
        n_iter += 1
        if n_iter >= miniter and history[-1] <= tol:
            converged = True
            break
        c = cast(apply_A(p), real)
        pc = wdot(p, c, weights, real)
        alpha = gamma / pc
        x = cast(proj([u + alpha * v for u, v in zip(x, p)]), real)
        r = cast(proj([u - alpha * v for u, v in zip(r, c)]), real)
        history.append(np.sqrt(wdot(r, r, weights, real)))
        c = cast(precon(r), real)
        gamma_new = wdot(r, c, weights, real)
        beta = gamma_new / gamma
        gamma = gamma_new
        p = cast(proj([u + beta * v for u, v in zip(c, p)]), real)
        alphas.append(alpha)
        betas.append(beta)
        if not pc > 0:
            negative = True
            break
    return dict(x=x, r=r, p=p, converged=converged, negative_curvature=negative, n_iter=n_iter, residual_norms=history,
                alphas=alphas, betas=betas)


class CgScalars:
    """The scalar side of the recursion as the C ABI cuts it: three named slots; GAMMA holds the NEXT gamma from a ``dot``
    until ``update_p`` makes it the current one."""

    def __init__(self, weights, real=LD):
        self.w, self.real = list(weights), real
        zero = real(0)
        self.gamma, self.gamma_next, self.pc, self.rr = zero, zero, zero, zero
        self.alpha = self.beta = None

    def dot(self, slot, a, b):
        v = wdot(a, b, self.w, self.real)
        if slot == GAMMA:
            self.gamma_next = v
        elif slot == PC:
            self.pc = v
        elif slot == RR:
            self.rr = v
        else:
            raise ValueError("slot")
        return v

    def update_xr(self, p, c, x, r):
        """-> (x + alpha p, r - alpha c) with alpha = gamma / <p, c> from the slots"""
        self.alpha = self.gamma / self.pc
        p, c, x, r = (cast(v, self.real) for v in (p, c, x, r))
        return ([u + self.alpha * v for u, v in zip(x, p)], [u - self.alpha * v for u, v in zip(r, c)])

    def update_p(self, z, p, first=False):
        """-> z + beta p with beta = next gamma / gamma (first: z itself); the next gamma becomes the current one"""
        z = cast(z, self.real)
        if first:
            out = [u.copy() for u in z]
        else:
            self.beta = self.gamma_next / self.gamma
            out = [u + self.beta * v for u, v in zip(z, cast(p, self.real))]
        self.gamma = self.gamma_next
        return out

    def read(self):
        return self.rr, self.gamma, self.pc


def cg_in_pieces(apply_A, b, weights, precon=None, proj=None, tol=1e-10, maxiter=100, miniter=1, real=LD):
    """``cg`` driven through ``CgScalars`` in the order in which the device driver issues the calls"""
    precon = precon or (lambda v: [u.copy() for u in v])
    proj = proj or (lambda v: v)
    s = CgScalars(weights, real)
    r = cast(b, real)
    x = [np.zeros_like(u) for u in r]
    c = cast(precon(r), real)
    s.dot(GAMMA, r, c)
    s.dot(RR, r, r)
    p = s.update_p(c, None, first=True)
    rr, _, _ = s.read()
    history = [np.sqrt(rr)]
    n_iter, converged, negative = 0, False, False
    while n_iter < maxiter:
        n_iter += 1
        if n_iter >= miniter and history[-1] <= tol:
            converged = True
            break
        c = cast(apply_A(p), real)
        s.dot(PC, p, c)
        x, r = s.update_xr(p, c, x, r)
        x, r = cast(proj(x), real), cast(proj(r), real)
        s.dot(RR, r, r)
        c = cast(precon(r), real)
        s.dot(GAMMA, r, c)
        p = cast(proj(s.update_p(c, p)), real)
        rr, _, pc = s.read()
        history.append(np.sqrt(rr))
        if not pc > 0:
            negative = True
            break
    return dict(x=x, r=r, p=p, converged=converged, negative_curvature=negative, n_iter=n_iter, residual_norms=history)
