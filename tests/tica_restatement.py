"""Test-side restatement of TICA (K16, csrc/tica.hip and coarsegrainingvae_amd/tica.py) in plain numpy: the features in
float32 with the kernel's operation order -- ``sqrt((dx*dx + dy*dy) + dz*dz)``, every operation rounded, the same bits as
the device -- and everything after them in fp64, as sums over frames.  The fit is the same algebra as
``tica.fit_from_moments`` written on its own."""
import numpy as np

from gram_restatement import hist2


def features(xyz, pairs):
    """``[T,d]`` float32 distances of the atom pairs, the kernel's operation order."""
    x = np.asarray(xyz, dtype=np.float32)
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    dlt = x[:, p[:, 0], :] - x[:, p[:, 1], :]                                   # float32 subtraction
    dx, dy, dz = dlt[..., 0], dlt[..., 1], dlt[..., 2]
    s = (dx * dx + dy * dy) + dz * dz                                          # float32, each operation rounded
    assert s.dtype == np.float32
    return np.sqrt(s)                                                          # correctly rounded float32


def moments(xyz, pairs, lag, order="forward"):
    """The five sums of one segment in fp64, added frame by frame (``order``: ``forward``, ``reversed`` -- the same sums
    in the opposite frame order -- or ``einsum``, numpy's own order)."""
    f = features(xyz, pairs).astype(np.float64)
    T, d = f.shape
    N = max(T - lag, 0)
    out = {"sum_x": np.zeros(d), "sum_y": np.zeros(d), "cxx": np.zeros((d, d)), "cyy": np.zeros((d, d)), "cxy": np.zeros((d, d)),
           "n_frame_pairs": N}
    if N == 0:
        return out
    x, y = f[:N], f[lag:lag + N]
    if order == "einsum":
        out.update(sum_x=x.sum(0), sum_y=y.sum(0), cxx=np.einsum("ti,tj->ij", x, x), cyy=np.einsum("ti,tj->ij", y, y),
                   cxy=np.einsum("ti,tj->ij", x, y))
        return out
    for t in (range(N) if order == "forward" else range(N - 1, -1, -1)):
        out["sum_x"] += x[t]
        out["sum_y"] += y[t]
        out["cxx"] += np.outer(x[t], x[t])
        out["cyy"] += np.outer(y[t], y[t])
        out["cxy"] += np.outer(x[t], y[t])
    return out


def add(a, b):
    return {k: a[k] + b[k] for k in a}


def fit(m, lag, dim=2, epsilon=1e-6):
    """``(mean, W, eigenvalues, rank)`` of the symmetrised estimator."""
    N = float(m["n_frame_pairs"])
    mean = 0.5 * (m["sum_x"] + m["sum_y"]) / N
    c0 = 0.5 * (m["cxx"] + m["cyy"]) / N - mean[:, None] * mean[None, :]
    ct = 0.5 * (m["cxy"] + m["cxy"].T) / N - mean[:, None] * mean[None, :]
    lam, q = np.linalg.eigh(c0)
    idx = [i for i in range(len(lam)) if lam[i] > epsilon * lam[-1]]
    white = np.stack([q[:, i] / np.sqrt(lam[i]) for i in idx], axis=1)
    ev, v = np.linalg.eigh(white.T @ ct @ white)
    ev, v = ev[::-1], v[:, ::-1]
    W = white @ v[:, :dim]
    for c in range(W.shape[1]):
        if W[np.argmax(np.abs(W[:, c])), c] < 0:
            W[:, c] = -W[:, c]
    return mean, W, ev[:W.shape[1]], len(idx)


def project(xyz, pairs, mean, W):
    """``(ics [S,k], mass [S,k])``: the components and ``sum_f |(f - mean)_f W_fc|``, the scale of their rounding error."""
    g = features(xyz, pairs).astype(np.float64) - np.asarray(mean, np.float64)[None, :]
    W = np.asarray(W, np.float64)
    return g @ W, np.abs(g) @ np.abs(W)


def bin2(ics, ca, cb, nb, ra, rb):
    """Host binning of components: ``(counts [nb,nb], outside)``; ``floor((v - lo) * nb / (hi - lo))`` in that order."""
    ics = np.asarray(ics, np.float64)
    return hist2(ics[:, ca], ics[:, cb], ra, rb, nb)


def hinge_chain(T, seed=0, phi=0.995, jitter=0.05, frozen=False):
    """A 12-atom chain of two straight arms (bond 1.5 A) joined at atom 5; the hinge angle follows an AR(1) path between
    two wells (60 and 120 degrees: the sign of the AR(1) variable picks the well, its size moves within it); every atom
    gets iid Gaussian jitter.  ``frozen``: the hinge stays in the first well.  Returns ``(xyz [T,12,3] float32, angle [T])``."""
    rng = np.random.default_rng(seed)
    u = np.empty(T)
    u[0] = 0.0
    noise = rng.standard_normal(T) * np.sqrt(1.0 - phi * phi)
    for t in range(1, T):
        u[t] = phi * u[t - 1] + noise[t]
    angle = np.radians(90.0 + 30.0 * np.tanh(3.0 * u) + 4.0 * u)
    if frozen:
        angle = np.radians(60.0 - 4.0 * np.abs(u))
    xyz = np.zeros((T, 12, 3))
    for a in range(6):
        xyz[:, a, 0] = -1.5 * (5 - a)                                          # the fixed arm along -x, atom 5 at the origin
    for a in range(6, 12):
        r = 1.5 * (a - 5)
        xyz[:, a, 0] = -r * np.cos(angle)                                      # angle between the arms at the hinge
        xyz[:, a, 1] = r * np.sin(angle)
    xyz += jitter * rng.standard_normal(xyz.shape)
    return xyz.astype(np.float32), angle
