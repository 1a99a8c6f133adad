"""numpy float64 restatements of cleanfid's frechet_distance and kernel_distance (from their published formulas; cleanfid and
scipy are not needed): the references of test_fid_cpu.py / test_fid_gpu.py."""
import numpy as np


def moments(f):
    """(mu, sigma) as cleanfid takes them: np.mean(axis=0), np.cov(rowvar=False)"""
    f = np.asarray(f, np.float64)
    return f.mean(axis=0), np.atleast_2d(np.cov(f, rowvar=False))


def trace_sqrt_eigh(s1, s2):
    """tr sqrt(S1 S2) through R = S1^(1/2) (eigh) and the eigenvalues of R S2 R, negative ones clipped"""
    w, v = np.linalg.eigh(s1)
    r = (v * np.sqrt(np.clip(w, 0, None))) @ v.T
    m = r @ s2 @ r
    return float(np.sqrt(np.clip(np.linalg.eigvalsh((m + m.T) / 2), 0, None)).sum())


def trace_sqrt_svd(f1, f2):
    """tr sqrt(S1 S2) = ||A B^T||_* / sqrt((N1 - 1)(N2 - 1)), A, B the centred features: exact for singular covariances"""
    f1, f2 = np.asarray(f1, np.float64), np.asarray(f2, np.float64)
    a, b = f1 - f1.mean(axis=0), f2 - f2.mean(axis=0)
    s = np.linalg.svd(a @ b.T, compute_uv=False)
    return float(s.sum() / np.sqrt((len(f1) - 1.0) * (len(f2) - 1.0)))


def frechet_distance(f1, f2, form="eigh"):
    mu1, s1 = moments(f1)
    mu2, s2 = moments(f2)
    diff = mu1 - mu2
    tr = trace_sqrt_eigh(s1, s2) if form == "eigh" else trace_sqrt_svd(f1, f2)
    return float(diff.dot(diff) + np.trace(s1) + np.trace(s2) - 2 * tr)


def kernel_distance(feats1, feats2, num_subsets=100, max_subset_size=1000):
    """cleanfid's loop as written, on numpy's global generator (the caller seeds it); also returns max |k| of the subsets"""
    feats1, feats2 = np.asarray(feats1, np.float64), np.asarray(feats2, np.float64)
    n = feats1.shape[1]
    m = min(min(feats1.shape[0], feats2.shape[0]), max_subset_size)
    t = 0
    kmax = 0.0
    for _subset_idx in range(num_subsets):
        x = feats2[np.random.choice(feats2.shape[0], m, replace=False)]
        y = feats1[np.random.choice(feats1.shape[0], m, replace=False)]
        a = (x @ x.T / n + 1) ** 3 + (y @ y.T / n + 1) ** 3
        b = (x @ y.T / n + 1) ** 3
        t += (a.sum() - np.diag(a).sum()) / (m - 1) - b.sum() * 2 / m
        kmax = max(kmax, float(np.abs((x @ x.T / n + 1) ** 3).max()), float(np.abs((y @ y.T / n + 1) ** 3).max()),
                   float(np.abs(b).max()))
    return float(t / num_subsets / m), kmax
