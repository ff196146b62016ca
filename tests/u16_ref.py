"""fp64 numpy restatement of the 16-bit grey bilateral kernel (GLF_KERNEL_BILATERAL_U16) and of the stages built on it, for the tests:

    K(i, j) = exp(-((r_i - r_j)^2 + (c_i - c_j)^2) / h_loc^2) exp(-(v_i - v_j)^2 / h_val^2),   v in 0..65535

Pixel indices are raster indices (row = idx // width, column = idx % width); images are uint16 [height, width]."""
import numpy as np


def _coords(w, idx):
    idx = np.asarray(idx, dtype=np.int64)
    return (idx // w).astype(np.float64), (idx % w).astype(np.float64)


def kernel(img, idx_a, idx_b, h_loc, h_val):
    """K(a, b) for pixel index lists a, b: float64 [len(a), len(b)]."""
    h, w = img.shape
    flat = img.reshape(-1).astype(np.float64)
    ra, ca = _coords(w, idx_a)
    rb, cb = _coords(w, idx_b)
    d2 = (ra[:, None] - rb[None, :]) ** 2 + (ca[:, None] - cb[None, :]) ** 2
    dv = flat[np.asarray(idx_a)][:, None] - flat[np.asarray(idx_b)][None, :]
    return np.exp(-d2 / (float(h_loc) ** 2) - dv * dv / (float(h_val) ** 2))


def degree(img, idx, h_loc, h_val, chunk=4096):
    """D_A[i] = sum over every pixel of K(sample i, pixel) (the row sums of [K_A K_B])."""
    n = img.size
    d = np.zeros(len(idx))
    for p0 in range(0, n, chunk):
        d += kernel(img, idx, np.arange(p0, min(n, p0 + chunk)), h_loc, h_val).sum(axis=1)
    return d


def laplacian(img, idx, h_loc, h_val):
    """(K_A, D_A, alpha, L_A = alpha (diag(D_A) - K_A)), alpha = 1 / mean(D_A)."""
    KA = kernel(img, idx, idx, h_loc, h_val)
    D = degree(img, idx, h_loc, h_val)
    alpha = 1.0 / D.mean()
    return KA, D, alpha, alpha * (np.diag(D) - KA)


def phi_rows(img, idx, pixels, phi_A, lam, alpha, h_loc, h_val):
    """Rows of the Nystroem extension Phi for the given pixels: the sample's Phi_A row at a sample pixel, else
    -alpha K(samples, pixel)^T Phi_A diag(1 / lam). phi_A: [p, m], lam: [m]."""
    pixels = np.asarray(pixels, dtype=np.int64)
    psi = -alpha * np.asarray(phi_A, dtype=np.float64) / np.asarray(lam, dtype=np.float64)[None, :]
    out = kernel(img, idx, pixels, h_loc, h_val).T @ psi
    pos = {int(v): i for i, v in enumerate(idx)}
    for k, px in enumerate(pixels):
        if int(px) in pos:
            out[k] = phi_A[pos[int(px)]]
    return out


def weights(phi, lam, mode, c, beta=1.5):
    """The filter's weights w (z - (1 - ysub) x = gain Phi w) from c = Phi^T x: f(Pi) c, or the sharpening filter's
    (1 + beta) L G L c - beta L G L G L c with L = diag(1 - mu) and G = Phi^T Phi."""
    lam = np.asarray(lam, dtype=np.float64)
    if mode == 0:
        return lam * c
    if mode == 1:
        return -(lam + 5.0) * c
    s = 1.0 - lam
    if mode == 2:
        return s * c
    G = phi.T @ phi
    u = s * (G @ (s * c))
    v = s * (G @ u)
    return (1.0 + beta) * u - beta * v


def correction(img, phi, lam, mode, gain):
    """z - (1 - ysub) x: float64 [N]. phi: the raster-order [N, m] extension."""
    x = img.reshape(-1).astype(np.float64)
    g = gain if mode == 0 else 1.0
    return g * (phi @ weights(phi, lam, mode, phi.T @ x))
