"""numpy restatement of the Moving MNIST rule of include/mmvae.h (mmvae_generate_clips), for the generator's tests.

Everything is the rule as written there, in the order written there: uint64 draws with wrap-around, an int32 velocity table computed in
f64, int32 trajectories that update first and record afterwards, frames composited with max.  Plain loops; no cleverness."""
import numpy as np

MASK = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15
ONE = 65536


def mix64(z):
    z &= MASK
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & MASK
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & MASK
    z ^= z >> 31
    return z


def draws(seed, c, k, D):
    """(glyph, x, y, direction) of digit k of clip c."""
    n = (8 * c + k) & MASK
    r1 = mix64(seed + GOLD * (2 * n + 1))
    r2 = mix64(seed + GOLD * (2 * n + 2))
    return ((r1 >> 32) * D) >> 32, r2 & 0xFFFF, (r2 >> 16) & 0xFFFF, (r2 >> 32) & 0xFFF


def velocity_table(speed):
    a = np.arange(4096, dtype=np.float64)
    vx = np.rint(speed * 65536.0 * np.cos(2.0 * np.pi * a / 4096.0))
    vy = np.rint(speed * 65536.0 * np.sin(2.0 * np.pi * a / 4096.0))
    return np.stack([vx, vy], axis=1).astype(np.int32)


def trajectory(x, y, vx, vy, T, R):
    """[(px, py)] for t = 0 .. T-1 and the number of bounces."""
    out, bounces = [], 0
    for _ in range(T):
        x += vx
        y += vy
        if x <= 0:
            x, vx, bounces = 0, -vx, bounces + 1
        if x >= ONE:
            x, vx, bounces = ONE, -vx, bounces + 1
        if y <= 0:
            y, vy, bounces = 0, -vy, bounces + 1
        if y >= ONE:
            y, vy, bounces = ONE, -vy, bounces + 1
        out.append(((x * R) >> 16, (y * R) >> 16))
    return out, bounces


def generate(bank, n_clips, seed, first_clip=0, frames=20, canvas=64, digits=2, speed=0.1, info=None):
    """uint8 (n_clips, frames, canvas, canvas).  ``info`` (a dict) receives 'positions' [(clip, digit, t, px, py)], 'bounces' (total)
    and 'overlaps' (pixels where two glyphs are both non-zero)."""
    bank = np.asarray(bank)
    D, G = bank.shape[0], bank.shape[1]
    R = canvas - G
    vel = velocity_table(speed)
    out = np.zeros((n_clips, frames, canvas, canvas), dtype=np.uint8)
    positions, bounces, overlaps = [], 0, 0
    for i in range(n_clips):
        c = first_clip + i
        covered = np.zeros((frames, canvas, canvas), dtype=np.int32)
        for k in range(digits):
            g, x, y, a = draws(seed, c, k, D)
            path, b = trajectory(int(x), int(y), int(vel[a, 0]), int(vel[a, 1]), frames, R)
            bounces += b
            for t, (px, py) in enumerate(path):
                positions.append((c, k, t, px, py))
                window = out[i, t, py:py + G, px:px + G]
                np.maximum(window, bank[g], out=window)
                covered[t, py:py + G, px:px + G] += bank[g] > 0
        overlaps += int((covered > 1).sum())
    if info is not None:
        info.update(positions=positions, bounces=bounces, overlaps=overlaps)
    return out
