"""Statistics of the P_N+ prior of the W+ loop (II2S: Zhu et al., "Improved StyleGAN Embedding: Where are the Good Latents?").

The mapping network ends in a LeakyReLU(0.2); x = l5(w), l5(t) = t if t > 0 else 5 t, undoes it, and the PCA of x over the mapping network's
own outputs whitens it: P_N.  The prior is the squared length there, the Mahalanobis distance of l5(w) to the distribution the generator was
trained on, per latent row (P_N+).  Statistics, once per set of mapping weights (``pn_stats``; ``Generator.pn_stats`` caches them):

    z ~ N(0, I): n rows drawn on the CPU from ONE torch.Generator().manual_seed(seed), consumed in consecutive chunks of PN_CHUNK rows — the
    chunking is part of the definition, so the values do not depend on the device; per chunk w = style(z) on the device, x = l5(w);
    sum x and sum x x^T in float64;  mu = mean;  Sigma = the covariance with n - 1 in the denominator;  sigma^2, C = eigh(Sigma) in float64;
    sigma^2_k <- max(sigma^2_k, floor * max sigma^2);  M = C diag(1 / sigma^2) C^T in float64, rounded to float32 once.

Term, per image: q = l5(w) - mu per row, pn_b = mean over the L rows and D columns of q^T M q — II2S's ``latent_p_norm.pow(2).mean()`` with
latent_p_norm = (l5(w) - X_mean) X_comp^T / X_stdev.  tests/pn_ref.py restates all of it independently in float64."""
import torch

PN_CHUNK = 10000


def leaky5(w):
    """l5(w): t for t > 0, 5 t otherwise — the inverse of LeakyReLU(0.2)."""
    return torch.where(w > 0, w, 5.0 * w)


class PNStats:
    """What the P_N+ term needs: ``mean`` (D,) and ``matrix`` (D, D), float32 on the device the kernel runs on; ``mean64`` (D,), ``components``
    (D, D: the eigenvectors as columns) and ``variance`` (D,: after flooring), float64 on the CPU; ``n``, ``seed``, ``floor`` as given."""

    def __init__(self, mean64, components, variance, n, seed, floor, device=None, _dev=None):
        self.mean64, self.components, self.variance = mean64, components, variance
        self.n, self.seed, self.floor = int(n), int(seed), float(floor)
        if _dev is None:
            matrix = (components / variance) @ components.T
            _dev = (mean64.float().contiguous(), (0.5 * (matrix + matrix.T)).float().contiguous())     # symmetric to the bit
        self.mean, self.matrix = (t if device is None else t.to(device).contiguous() for t in _dev)

    @property
    def dim(self):
        return int(self.mean64.numel())

    def to(self, device):
        """The same statistics with ``mean`` and ``matrix`` on ``device`` (the float64 parts stay on the CPU and are shared)."""
        if torch.device(device) == self.mean.device:
            return self
        return PNStats(self.mean64, self.components, self.variance, self.n, self.seed, self.floor, device, (self.mean, self.matrix))

    def distance(self, w):
        """pn_b of ``w`` (B, L, D) or (B, D), float64 (B,) on the host, from the float64 statistics — for reporting."""
        x = w.detach().double().cpu()
        if x.dim() < 2 or x.shape[-1] != self.dim:
            raise ValueError(f'PNStats.distance: w must be (B, ..., {self.dim}), got {tuple(w.shape)}')
        p = (leaky5(x) - self.mean64) @ self.components
        return (p * p / self.variance).reshape(x.shape[0], -1).mean(1)


def pn_stats(style, dim, device, n=100000, seed=0, floor=0.0):
    """The statistics of the module docstring for the mapping ``style`` (a callable (c, dim) float32 on ``device`` -> the same shape), as a
    ``PNStats`` on ``device``.  ValueError for n < 2, a negative or non-finite floor, and for a variance that is not positive after
    flooring — n <= dim with floor 0; 'not positive' is taken up to float64 rounding, sigma^2_k <= dim * 2^-52 * max sigma^2."""
    n, seed, floor = int(n), int(seed), float(floor)
    if n < 2:
        raise ValueError(f'pn_samples must be at least 2, got {n}')
    if not (floor >= 0.0 and floor < float('inf')):
        raise ValueError(f'pn_floor must be a finite number >= 0, got {floor!r}')
    gen = torch.Generator().manual_seed(seed)
    s1 = torch.zeros(dim, dtype=torch.float64, device=device)
    s2 = torch.zeros(dim, dim, dtype=torch.float64, device=device)
    with torch.no_grad():
        for c0 in range(0, n, PN_CHUNK):
            z = torch.randn(min(PN_CHUNK, n - c0), dim, generator=gen)
            x = leaky5(style(z.to(device)).double())         # the factor 5 applied in float64: no rounding of its own
            s1 += x.sum(0)
            s2 += x.T @ x
    s1, s2 = s1.cpu(), s2.cpu()
    mean = s1 / n
    cov = (s2 - n * torch.outer(mean, mean)) / (n - 1)
    var, comp = torch.linalg.eigh(0.5 * (cov + cov.T))
    top = float(var.max())
    var = torch.clamp(var, min=floor * top)
    if not bool((var > dim * 2.0 ** -52 * top).all()):
        raise ValueError(f'P_N statistics: {int((var <= dim * 2.0 ** -52 * top).sum())} of {dim} variances are not positive with pn_samples = {n} and '
                         f'pn_floor = {floor}: draw more than {dim} samples, or give pn_floor > 0')
    return PNStats(mean, comp, var, n, seed, floor, device)
