"""NumPy twin of the optimiser of direct_minimization (csrc/dm_kernels.hip): the L-BFGS update rule and the two-loop
recursion on packed vectors (lists of complex (n_rows, n_cols) arrays), in ``numpy.longdouble`` (the reference of the kernel
tests) or in float64 (the yardstick of their bound: the tests allow 64 x the error the float64 twin makes against the
longdouble one); the dense forms of the Stiefel helpers; the explicit BFGS recursion the two-loop form is checked against.
"""
import numpy as np

LD = np.longdouble
CLD = np.clongdouble


def cast(v, real):
    return [np.asarray(b).astype(CLD if real is LD else np.complex128) for b in v]


def dot(a, b):
    """Optim's inner product: sum over blocks and entries of Re(conj(a) b)"""
    return sum((x.real * y.real).sum() + (x.imag * y.imag).sum() for x, y in zip(a, b))


def middle(q, scale, kin=None, mean_kin=None):
    """the preconditioner step of the recursion: kin-wise mean_kin / (mean_kin + kin) (PreconditionerTPA ldiv!), then / scale"""
    out = []
    for b, x in enumerate(q):
        if kin is not None:
            f = mean_kin[b][None, :] / (mean_kin[b][None, :] + kin[b][:, None])
            x = x * f
        out.append(x / scale[b])
    return out


class LbfgsTwin:
    def __init__(self, memory, real=LD):
        self.memory, self.real = int(memory), real
        self.pairs = []                  # (s, y, rho), oldest first
        self.prev = None

    def reset(self):
        self.pairs, self.prev = [], None

    def update(self, x, g):
        x, g = cast(x, self.real), cast(g, self.real)
        if self.prev is None:
            self.prev = (x, g)
            return 0.0, False
        s = [a - b for a, b in zip(x, self.prev[0])]
        y = [a - b for a, b in zip(g, self.prev[1])]
        self.prev = (x, g)
        sy = dot(s, y)
        if not (np.isfinite(sy) and sy > 0):
            return float(sy), False
        self.pairs.append((s, y, 1 / sy))
        self.pairs = self.pairs[-self.memory:]
        return float(sy), True

    def direction(self, g, scale, kin=None, mean_kin=None):
        real = self.real
        q = cast(g, real)
        scale = [real(s) for s in scale]
        if kin is not None:
            kin = [np.asarray(k).astype(real) for k in kin]
            mean_kin = [np.asarray(m).astype(real) for m in mean_kin]
        alpha = []
        peak = lambda v: max(float(np.abs(b).max()) for b in v)      # noqa: E731
        self.peak_q = peak(q)            # the largest entry of any intermediate vector before / after the middle step
        for s, y, rho in reversed(self.pairs):
            a = rho * dot(s, q)
            q = [u - a * v for u, v in zip(q, y)]
            alpha.append(a)
            self.peak_q = max(self.peak_q, peak(q))
        r = middle(q, scale, kin, mean_kin)
        self.peak_r = peak(r)
        for (s, y, rho), a in zip(self.pairs, reversed(alpha)):
            beta = rho * dot(y, r)
            r = [u + (a - beta) * v for u, v in zip(r, s)]
            self.peak_r = max(self.peak_r, peak(r))
        return [-u for u in r]


# ---- the explicit recursion on real vectors ------------------------------------------------------------------------------
def flatten(v):
    """packed vector -> one real vector (real parts, then imaginary parts, of every block); dot() becomes the plain one"""
    return np.concatenate([np.concatenate([np.asarray(b).real.ravel(), np.asarray(b).imag.ravel()]) for b in v])


def explicit_bfgs_direction(pairs, H0_diag, g):
    """-H g with H <- (I - rho s y') H (I - rho y s') + rho s s' over the pairs (oldest first), H = diag(H0_diag) at the
    start; all real vectors (longdouble)."""
    n = len(g)
    H = np.diag(np.asarray(H0_diag, dtype=LD))
    I = np.eye(n, dtype=LD)
    for s, y in pairs:
        rho = 1 / (s @ y)
        H = (I - rho * np.outer(s, y)) @ H @ (I - rho * np.outer(y, s)) + rho * np.outer(s, s)
    return -(H @ g)


# ---- Stiefel manifold, dense ---------------------------------------------------------------------------------------------
def project_tangent(g, x):
    """Optim's project_tangent!(Stiefel(), g, x): g - x (x'g + g'x) / 2"""
    xg = x.conj().T @ g
    return g - x @ ((xg + xg.conj().T) / 2)


def polar_retract(x):
    """Optim's retract!(Stiefel(), x): the polar factor U V' of x = U S V'"""
    u, _, vh = np.linalg.svd(x, full_matrices=False)
    return u @ vh
