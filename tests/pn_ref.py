"""The P_N+ prior of the W+ loop (II2S, Zhu et al.: "Improved StyleGAN Embedding: Where are the Good Latents?") restated in plain
torch, float64: the yardstick of tests/test_pn_prior_cpu.py, tests/test_hip_pn_prior.py and tests/golden/make_wplus_pn.py.  Nothing here
imports the package.

Statistics: z ~ N(0, I), n rows from ONE torch.Generator().manual_seed(seed) on the CPU, consumed in consecutive chunks of 10000 rows; per chunk
w = style(z), x = l5(w), l5(t) = t if t > 0 else 5 t; sum x and sum x x^T in float64; mu = mean; Sigma = covariance with n - 1; sigma^2, C =
eigh(Sigma); sigma^2_k <- max(sigma^2_k, floor * max sigma^2); a variance that is not positive afterwards raises.
Term: q = l5(w) - mu per latent row, p = q C / sigma (II2S's latent_p_norm), pn_b = mean over rows and columns of p^2 = mean q^T M q with
M = C diag(1 / sigma^2) C^T."""
import torch
import torch.nn.functional as F

CHUNK = 10000


def leaky5(w):
    """l5 through torch's own leaky_relu, so that autograd gives its backward: slope 5 for t <= 0, 0 included."""
    return F.leaky_relu(w, 5.0)


def stats(style, dim, n, seed=0, floor=0.0, device='cpu'):
    """dict(mean (D,), components (D, D: eigenvectors as columns), variance (D,: floored), matrix (D, D)), float64 on the CPU, for the mapping
    ``style`` (a callable on (c, dim) float32 tensors on ``device``)."""
    gen = torch.Generator().manual_seed(int(seed))
    s1 = torch.zeros(dim, dtype=torch.float64)
    s2 = torch.zeros(dim, dim, dtype=torch.float64)
    with torch.no_grad():
        for c0 in range(0, n, CHUNK):
            z = torch.randn(min(CHUNK, n - c0), dim, generator=gen)
            x = leaky5(style(z.to(device)).double().cpu())
            s1 += x.sum(0)
            s2 += x.T @ x
    mean = s1 / n
    cov = (s2 - n * torch.outer(mean, mean)) / (n - 1)
    var, comp = torch.linalg.eigh(0.5 * (cov + cov.T))
    top = var.max().item()
    var = torch.clamp(var, min=floor * top)
    # "not positive" up to float64 rounding: a rank-deficient covariance (n <= D) has eigenvalues of either sign at dim * 2^-52 * max
    if not bool((var > dim * 2.0 ** -52 * top).all()):
        raise ValueError(f'pn_ref.stats: variances that are not positive with pn_samples = {n}, pn_floor = {floor}')
    return dict(mean=mean, components=comp, variance=var, matrix=(comp / var) @ comp.T)


def synthetic_stats(dim, seed=0):
    """Statistics with the spread a real mapping network shows (the seeded 8-layer mapping network of oodgan.synth, n = 20000: largest over
    smallest eigenvalue 5e7, none <= 0): a seeded orthogonal C from a float64 QR, eigenvalues log-spaced over 1e-7 ... 1e2, mu = randn."""
    gen = torch.Generator().manual_seed(int(seed))
    comp, _ = torch.linalg.qr(torch.randn(dim, dim, generator=gen, dtype=torch.float64))
    var = torch.logspace(-7, 2, dim, dtype=torch.float64) if dim > 1 else torch.ones(1, dtype=torch.float64)
    mean = torch.randn(dim, generator=gen, dtype=torch.float64)
    return dict(mean=mean, components=comp, variance=var, matrix=(comp / var) @ comp.T)


def sample(st, shape, seed=0, spread=0.3):
    """Latents w (float32, ``shape`` = (..., D)): on-distribution samples l5^-1(mu + C (sigma z)) plus ``spread`` * randn — many negative
    entries, off-distribution along the directions of small variance."""
    gen = torch.Generator().manual_seed(int(seed))
    z = torch.randn(*shape, generator=gen, dtype=torch.float64)
    x = st['mean'] + (z * st['variance'].sqrt()) @ st['components'].T
    w = F.leaky_relu(x, 0.2) + spread * torch.randn(*shape, generator=gen, dtype=torch.float64)
    return w.float()


def term(w, st):
    """pn_b (B,) of w (B, L, D) or (B, D) in w's dtype through the whitened coordinates (differentiable): II2S's latent_p_norm.pow(2).mean()."""
    dt = w.dtype
    p = (leaky5(w) - st['mean'].to(dt)) @ st['components'].to(dt) / st['variance'].to(dt).sqrt()
    return (p * p).reshape(w.shape[0], -1).mean(1)


def term_matrix(w, mean, matrix):
    """The same value as the quadratic form q^T M q the kernel evaluates, in the dtype of its arguments (differentiable): the plain-torch
    restatement whose own fp32 error sets the kernel's bars."""
    q = leaky5(w) - mean
    return (q * (q @ matrix)).reshape(w.shape[0], -1).mean(1)
