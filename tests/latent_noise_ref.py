"""The latent noise of the W+ loop (include/oodgan.h, oodgan_latent_noise) restated with numpy integers and float64: the
yardstick of tests/test_hip_wplus_sched.py, itself pinned by the Philox known answers in tests/test_wplus_sched_cpu.py.

    n(seed, id, i, e) = value e & 3 of the two Box-Muller pairs made from Philox4x32-10(key = (seed lo, seed hi),
                                                                                      counter = (e >> 2, id lo, i, id hi))"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or ints) of one shape, key: two -> the four output words as uint64 arrays holding 32-bit values."""
    c = [np.asarray(x, dtype=np.uint64) & _MASK for x in np.broadcast_arrays(*[np.asarray(x, dtype=np.uint64) for x in counter])]
    k = [int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]                # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k[0]), p1 & _MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k[1]), p0 & _MASK]
        k = [(k[0] + W0) & 0xFFFFFFFF, (k[1] + W1) & 0xFFFFFFFF]
    return c


def uniforms(words):
    """u_k = ((x_k >> 8) + 0.5) 2^-24, in (0, 1), float64."""
    return [((x >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24 for x in words]


def unit_normals(seed, image_id, step, n):
    """n(seed, image_id, step, e) for e = 0 .. n-1, float64 (n,)."""
    seed, image_id = int(seed), int(image_id)
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    x = philox4x32_10((q, image_id & 0xFFFFFFFF, int(step), (image_id >> 32) & 0xFFFFFFFF), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    u = uniforms(x)
    r0, r1 = np.sqrt(-2.0 * np.log(u[0])), np.sqrt(-2.0 * np.log(u[2]))
    a0, a1 = 2.0 * np.pi * u[1], 2.0 * np.pi * u[3]
    vals = np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1)], 1)
    return vals.reshape(-1)[:n]


def sigma(step, total_steps, sigma0, noise_ramp):
    """sigma_i = sigma0 * max(0, 1 - (i / total_steps) / noise_ramp)^2; noise_ramp <= 0: sigma0."""
    if noise_ramp <= 0:
        return float(sigma0)
    return float(sigma0) * max(0.0, 1.0 - (step / total_steps) / noise_ramp) ** 2


def latent_noise(seed, ids, step, n, total_steps, sigma0, noise_ramp):
    """sigma_i * n for the images ``ids``: float64 (len(ids), n)."""
    s = sigma(step, total_steps, sigma0, noise_ramp)
    return np.stack([s * unit_normals(seed, i, step, n) for i in ids], 0)
