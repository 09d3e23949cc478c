"""Test-side restatement of the reference-free ensemble checks (K14, csrc/ensemble_check.hip) with dense matrices, and
the hand-built molecule its tests use.  It lives in the tests only: nothing on the product path imports it, and it is no
fallback for a missing kernel.

Written independently of the kernel: the inferred bond graph is a dense boolean ``[n,n]`` matrix from fp32 distances in
the ``.pow(2).sum(-1)`` operation order and ``s <= thr_sq``; the topology is a dense boolean matrix; missing / extra are
SET DIFFERENCES of the two (not the kernel's ``Eb - H`` / ``P - H`` counting); the pair sums are fp64.
"""
import numpy as np
import torch

from coarsegrainingvae_amd import evaluate as ev


def restate(gen, z, frame_ptr, K, bonds, bond_ptr=None, radii=None, scale=1.3):
    """``counts [B,K,4]`` int64 and ``pair_sums [B,K,K,2]`` float64 for ``gen [K*N,3]`` (frame-major, sample-major inside
    a frame), atomic numbers ``z [N]``, frame-local ``bonds`` (one list for every frame without ``bond_ptr``)."""
    gen = torch.as_tensor(np.asarray(gen), dtype=torch.float32)
    z = np.asarray(z).astype(np.int64)
    elements = sorted(set(z.tolist()))
    thr = ev.bond_thresholds(elements, scale, radii)
    cls = torch.from_numpy(np.searchsorted(elements, z))
    B = len(frame_ptr) - 1
    bonds = np.asarray(bonds, dtype=np.int64).reshape(-1, 2)
    counts = torch.zeros(B, K, 4, dtype=torch.int64)
    sums = torch.zeros(B, K, K, 2, dtype=torch.float64)
    for f in range(B):
        lo, hi = int(frame_ptr[f]), int(frame_ptr[f + 1])
        n = hi - lo
        mine = bonds if bond_ptr is None else bonds[int(bond_ptr[f]):int(bond_ptr[f + 1])]
        topo = torch.zeros(n, n, dtype=torch.bool)
        topo[mine[:, 0], mine[:, 1]] = True
        topo = topo | topo.t()
        h = torch.from_numpy(z[lo:hi] != 1)
        hh = h[:, None] & h[None, :]
        c = cls[lo:hi]
        xs = gen[K * lo:K * hi].reshape(K, n, 3)
        for k in range(K):
            d = xs[k][:, None, :] - xs[k][None, :, :]
            s = d.pow(2).sum(-1)                                        # fp32, (dx^2 + dy^2) + dz^2
            got = s <= thr[c[:, None], c[None, :]]
            got.fill_diagonal_(False)
            miss, extra = topo & ~got, got & ~topo
            counts[f, k] = torch.stack([miss.sum(), extra.sum(), (miss & hh).sum(), (extra & hh).sum()]) // 2
        d2 = (xs.double()[:, None] - xs.double()[None, :]).pow(2).sum(-1)       # [K,K,n]
        sums[f, ..., 0] = d2.sum(-1)
        sums[f, ..., 1] = d2[..., h].sum(-1)
    return counts, sums


# ----------------------------------------------------------------------------- the hand-built molecule
N_CARBON = 24
HALF = np.deg2rad(109.5) / 2
DX, DZ = 1.5 * np.sin(HALF), 1.5 * np.cos(HALF)          # zigzag step: 1-3 distance 2 DX = 2.45 A > the C-C cutoff 1.768


def alkane():
    """A zigzag carbon chain (1.5 A bonds, 109.5 degree angles) with hydrogens at 1.09 A, every carbon followed by its
    hydrogens: 74 atoms (a 64-atom tile boundary is crossed).  Returns ``xyz [74,3]`` float64, ``z [74]``,
    ``bonds [73,2]`` (i < j), ``carbon`` (atom index of every carbon)."""
    xyz, z, bonds, carbon = [], [], [], []
    for i in range(N_CARBON):
        c = np.array([i * DX, 0.0, (i % 2) * DZ])
        s = 1.0 if i % 2 else -1.0                         # hydrogens point away from the neighbours' side
        carbon.append(len(xyz))
        xyz.append(c), z.append(6)
        if i:
            bonds.append((carbon[i - 1], carbon[i]))
        hs = [c + 1.09 * np.array([0.0, sg * np.sin(HALF), s * np.cos(HALF)]) for sg in (1.0, -1.0)]
        if i == 0:
            hs.append(c + 1.09 * np.array([-np.sin(HALF), 0.0, np.cos(HALF)]))           # where carbon -1 would be
        if i == N_CARBON - 1:
            last_s = -s
            hs.append(c + 1.09 * np.array([np.sin(HALF), 0.0, last_s * np.cos(HALF)]))   # where carbon 24 would be
        for hpos in hs:
            bonds.append((carbon[i], len(xyz)))
            xyz.append(hpos), z.append(1)
    return np.array(xyz), np.array(z), np.array(bonds, dtype=np.int64), np.array(carbon)


def _sq32(d):
    d = np.asarray(d, dtype=np.float32)
    return np.float32(np.float32(d[0] * d[0]) + np.float32(d[1] * d[1]))        # + 0 * 0: dz = 0


def offset_with_sq(target):
    """An fp32 offset ``(dx, dy, 0)`` whose squared length, computed in fp32 as ``(dx*dx + dy*dy) + dz*dz``, is exactly
    the fp32 number ``target``."""
    target = np.float32(target)
    dx = np.float32(np.sqrt(np.float64(target)) * 0.999)
    for _ in range(4096):
        rem = np.float64(target) - np.float64(dx) * np.float64(dx)
        dy0 = np.float32(np.sqrt(rem))
        for step in range(-64, 65):
            dy = dy0
            for _s in range(abs(step)):
                dy = np.nextafter(dy, np.float32(np.inf if step > 0 else -np.inf), dtype=np.float32)
            if _sq32((dx, dy)) == target:
                return np.array([dx, dy, 0.0], dtype=np.float32)
        dx = np.nextafter(dx, np.float32(0), dtype=np.float32)
    raise RuntimeError("no fp32 offset reaches the target")


def cases():
    """``(names, gen [K,74,3] float32, z, bonds, expected counts [K,4])`` -- the expectations are reasoned by hand:
      valid        the unperturbed molecule                                        0 0 0 0
      stretched    carbons 12.. (with their hydrogens) moved 0.5 A along the bond 11-12: that bond is 2.0 A, everything
                   else moves apart                                                1 0 1 0
      pulled_in    the last CH3 translated so that C23 stays 1.5 A from C22 and comes to 1.7 A of C21 (< 1.768)
                                                                                   0 1 0 1
      hh_contact   the two hydrogens of carbon 6 closed to 0.5 A of each other (< the H-H cutoff 0.598), both still
                   1.09 A from their carbon                                        0 1 0 0
      at_thr       carbon 11 at the origin and the tail placed so that the fp32 squared length of bond 11-12 IS the
                   C-C threshold: still a bond                                     0 0 0 0
      above_thr    the same with the next fp32 number above the threshold: no bond  1 0 1 0
    """
    xyz, z, bonds, carbon = alkane()
    thr_cc = np.float32(float(ev.bond_thresholds([1, 6])[1, 1]))
    out, names, want = [], [], []

    def add(name, x, counts):
        names.append(name), out.append(np.asarray(x, dtype=np.float32)), want.append(counts)
    add("valid", xyz, (0, 0, 0, 0))
    x = xyz.copy()
    u = (xyz[carbon[12]] - xyz[carbon[11]]) / 1.5
    x[carbon[12]:] += 0.5 * u
    add("stretched", x, (1, 0, 1, 0))
    x = xyz.copy()
    c21, c22, c23 = xyz[carbon[21]], xyz[carbon[22]], xyz[carbon[23]]
    # in the chain's plane: 1.5 A from c22 at an angle phi from the direction c22 -> c21, 2 * 1.5 * sin(phi / 2) = 1.7
    phi = 2 * np.arcsin(1.7 / 3.0)
    e1 = (c21 - c22) / 1.5
    e2 = (c23 - c22) - np.dot(c23 - c22, e1) * e1
    e2 /= np.linalg.norm(e2)
    x[carbon[23]:] += (c22 + 1.5 * (np.cos(phi) * e1 + np.sin(phi) * e2)) - c23
    add("pulled_in", x, (0, 1, 0, 1))
    x = xyz.copy()
    c6, a = xyz[carbon[6]], np.arcsin(0.25 / 1.09)
    for sg, at in ((1.0, carbon[6] + 1), (-1.0, carbon[6] + 2)):
        x[at] = c6 + 1.09 * np.array([0.0, sg * np.sin(a), -np.cos(a)])            # carbon 6 is even: s = -1
    add("hh_contact", x, (0, 1, 0, 0))
    for name, target, counts in (("at_thr", thr_cc, (0, 0, 0, 0)),
                                 ("above_thr", np.nextafter(thr_cc, np.float32(np.inf), dtype=np.float32), (1, 0, 1, 0))):
        x = (xyz - xyz[carbon[11]]).astype(np.float32)                              # carbon 11 exactly at the origin
        off = offset_with_sq(target)
        # the tail moves with carbon 12, which lands exactly on `off`; pointing the offset along +x keeps the chain open
        x[carbon[12]:] = (x[carbon[12]:].astype(np.float64) - x[carbon[12]].astype(np.float64) + off.astype(np.float64)).astype(np.float32)
        x[carbon[12]] = off
        add(name, x, counts)
    return names, np.stack(out), z, bonds, np.array(want, dtype=np.int64)
