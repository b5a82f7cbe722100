"""Host mirror of RankUpdateEuclideanMetric (src/metric.jl:137-337, src/hamiltonian.jl:70-80,186-192): the arithmetic the device
path (include/ahmc_rank_update.h, csrc/ahmc_rank_update.hpp) implements, in numpy float64.

    M⁻¹ = W = Diagonal(A) + B·Dm·Bᵀ,   A (D,) > 0,   B (D, k),   Dm (k, k)

(the reference's k×k field `D` is `Dm` here, so that D keeps meaning the dimension).  `woodbury_factorize` is the reference's, with
LAPACK's Householder conventions (numpy's `qr(mode="raw")` is dgeqrf), and the compact-WY factor T of Q = I − Y·T·Yᵀ that the device
applies Q with, formed as LAPACK's dlarft forms it.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np


@dataclass
class WoodburyFactorization:
    """woodbury_factorize(A, B, D) (src/metric.jl:137-177): U = √A (the diagonal), Q from the thin QR U⁻¹B = Q·R as Householder
    vectors Y (D, k; unit diagonal, zeros above it) with τ and the compact-WY T, R (k, k), and V = chol(I + R·Dm·Rᵀ).U."""
    U: np.ndarray
    Y: np.ndarray
    tau: np.ndarray
    T: np.ndarray
    R: np.ndarray
    V: np.ndarray

    @property
    def k(self):
        return self.Y.shape[1]


def _larft(Y, tau):
    """T (k, k) upper triangular with H₁⋯H_k = I − Y·T·Yᵀ (dlarft, direct = 'F', storev = 'C')"""
    k = Y.shape[1]
    T = np.zeros((k, k))
    for i in range(k):
        if tau[i] == 0:
            continue
        w = -tau[i] * (Y[i:, :i].T @ Y[i:, i])
        T[:i, i] = T[:i, :i] @ w
        T[i, i] = tau[i]
    return T


def woodbury_factorize(A, B, Dm) -> WoodburyFactorization:
    A = np.asarray(A, dtype=np.float64).ravel()
    B = np.asarray(B, dtype=np.float64).reshape(A.size, -1)
    Dm = np.asarray(Dm, dtype=np.float64)
    D, k = B.shape
    U = np.sqrt(A)
    if k == 0:
        return WoodburyFactorization(U, np.zeros((D, 0)), np.zeros(0), np.zeros((0, 0)), np.zeros((0, 0)), np.zeros((0, 0)))
    h, tau = np.linalg.qr(B / U[:, None], mode="raw")
    H = h.T  # (D, k): R on and above the diagonal, the Householder vectors below it
    Y = np.tril(H, -1)
    Y[np.arange(k), np.arange(k)] = 1.0
    R = np.triu(H[:k, :])
    S = R @ Dm @ R.T + np.eye(k)
    S = np.triu(S) + np.triu(S, 1).T  # Symmetric(S): the upper triangle
    V = np.linalg.cholesky(S).T
    return WoodburyFactorization(U, Y, tau, _larft(Y, tau), R, V)


def dense(A, B, Dm):
    """W = Diagonal(A) + B·Dm·Bᵀ as a (D, D) matrix"""
    A = np.asarray(A, dtype=np.float64).ravel()
    B = np.asarray(B, dtype=np.float64).reshape(A.size, -1)
    return np.diag(A) + B @ np.asarray(Dm, dtype=np.float64) @ B.T


def diag_inv_metric(A, B, Dm):
    """_diag_inv_metric (src/metric.jl:262-267): diag(A) + [bᵢᵀ·Dm·bᵢ]"""
    A = np.asarray(A, dtype=np.float64).ravel()
    B = np.asarray(B, dtype=np.float64).reshape(A.size, -1)
    return A + np.einsum("ij,jk,ik->i", B, np.asarray(Dm, dtype=np.float64), B)


def dHdr(A, B, Dm, r):
    """∂H∂r(r) = A∘r + B·(Dm·(Bᵀr)) for a vector r or the columns of a (D, N) array (src/hamiltonian.jl:70-80)"""
    r = np.asarray(r, dtype=np.float64)
    A = np.asarray(A, dtype=np.float64).ravel()
    B = np.asarray(B, dtype=np.float64).reshape(A.size, -1)
    a = A if r.ndim == 1 else A[:, None]
    return a * r + B @ (np.asarray(Dm, dtype=np.float64) @ (B.T @ r))


def neg_energy(A, B, Dm, r):
    """−(rᵀA r + (Bᵀr)ᵀ Dm (Bᵀr))/2 per column (src/hamiltonian.jl:186-192)"""
    r = np.asarray(r, dtype=np.float64)
    A = np.asarray(A, dtype=np.float64).ravel()
    B = np.asarray(B, dtype=np.float64).reshape(A.size, -1)
    a = A if r.ndim == 1 else A[:, None]
    s = B.T @ r
    return -(np.sum(a * r * r, axis=0) + np.sum(s * (np.asarray(Dm, dtype=np.float64) @ s), axis=0)) / 2


def rand_momentum(f: WoodburyFactorization, z):
    """rand_momentum (src/metric.jl:322-337) applied to standard normals z (a vector or the columns of (D, N)):
    z[1:k] ← V⁻¹z[1:k];  z ← Q·z = z − Y·(T·(Yᵀz));  r = z ./ √A"""
    z = np.array(z, dtype=np.float64, copy=True)
    k = f.k
    U = f.U if z.ndim == 1 else f.U[:, None]
    if k:
        z[:k] = np.linalg.solve(f.V, z[:k])
        z = z - f.Y @ (f.T @ (f.Y.T @ z))
    return z / U


def momentum_map(f: WoodburyFactorization):
    """the (D, D) matrix L of rand_momentum (r = L·z): Cov(r) = L·Lᵀ = W⁻¹"""
    return rand_momentum(f, np.eye(f.U.size))


# ---------------------------------------------------------------------------------------------------------------------
# Low-rank mass-matrix adaptation (include/ahmc_lowrank_adapt.h, csrc/ahmc_lowrank_adapt.hpp): the estimator that fits
# M⁻¹ = Diagonal(A) + B·Dm·Bᵀ to the draws of all chains.  The reference has no adaptor for this metric; what follows is the
# definition the device kernels (push) and the engine's host code (fit) implement.  All of it is float64.
#
# A window keeps the pooled Welford / Chan state of the draws seen so far — n, μ (D), m2 (D) = Σ(x − μ)² — and, instead of the
# D×D scatter matrix a dense covariance would need, its product with a thin test matrix: Z (D, ℓ) = Σ(x − μ)(x − μ)ᵀ·W with
# W = Ω / s₀ row-wise, Ω (D, ℓ) standard normals (later: the previous window's eigenvectors plus fresh normals) and s₀ (D) the
# scaling the fit works in (the previous window's standard deviations).  Y = Z/(n−1)/s₀ is then C_s·Ω for the covariance C_s in
# s₀-scaled coordinates, which is all a single-pass Nyström approximation needs.
# ---------------------------------------------------------------------------------------------------------------------
LOWRANK_MAX_ELL = 40
LOWRANK_MAX_K = 32  # AHMC_RANK_UPDATE_MAX_K
LOWRANK_NMIN = 10   # wv_nmin: a window with fewer draws is not fitted


@dataclass
class LowRankState:
    k: int
    ell: int
    seed: int
    n: int
    mu: np.ndarray
    m2: np.ndarray
    Z: np.ndarray
    s0: np.ndarray
    Omega: np.ndarray
    n_fits: int = 0       # windows restarted so far: the counter of the fresh normals' stream
    V: np.ndarray = None  # (D, k) eigenvectors of the last fit (what the next window's Ω starts with)

    @property
    def W(self):
        return self.Omega / self.s0[:, None]


def lowrank_ell(D, k, oversample=8):
    return min(int(D), int(k) + int(oversample))


def lowrank_init(s0, k, oversample=8, seed=0, Omega=None) -> LowRankState:
    """the state of a fresh adaptor: s₀ = √diag(M⁻¹) of the metric it starts from; Ω standard normals (the engine draws its own:
    pass the Ω read back from it to follow it)"""
    s0 = np.array(s0, dtype=np.float64).ravel()
    D = s0.size
    if not 1 <= k <= min(D, LOWRANK_MAX_K):
        raise ValueError(f"rank k = {k} must be in 1..min(D, {LOWRANK_MAX_K})")
    ell = lowrank_ell(D, k, oversample)
    if oversample < 0 or ell > LOWRANK_MAX_ELL:
        raise ValueError(f"k + oversample = {k + oversample} must be in k..{LOWRANK_MAX_ELL}")
    if Omega is None:
        Omega = np.random.default_rng(seed).standard_normal((D, ell))
    Omega = np.array(Omega, dtype=np.float64).reshape(D, ell)
    return LowRankState(int(k), ell, int(seed), 0, np.zeros(D), np.zeros(D), np.zeros((D, ell)), s0, Omega)


def lowrank_push(st: LowRankState, X):
    """one batch X (D, N) — every chain's position at one iteration — merged into the window (Chan's pooled update, as
    dn_cov_push does for WelfordCov, projected on W)"""
    X = np.asarray(X, dtype=np.float64).reshape(st.mu.size, -1)
    N = X.shape[1]
    mb = X.sum(axis=1) / N
    Xc = X - mb[:, None]
    delta = mb - st.mu
    f = st.n * N / (st.n + N)
    W = st.W
    st.Z += Xc @ (Xc.T @ W) + f * np.outer(delta, delta @ W)
    st.m2 += np.sum(Xc * Xc, axis=1) + f * delta * delta
    st.mu += delta * (N / (st.n + N))
    st.n += N
    return st


def lowrank_fit(st: LowRankState, nmin=LOWRANK_NMIN):
    """(A, B, Dm) fitted to the window, or None while it holds fewer than `nmin` draws.  Leaves the eigenvectors in st.V."""
    n = st.n
    if n < max(nmin, 2):
        return None
    D, k = st.mu.size, st.k
    s0 = st.s0
    c = st.m2 / (n - 1) / (s0 * s0)            # diag(C_s)
    Y = st.Z / (n - 1) / s0[:, None]           # C_s·Ω
    G = st.Omega.T @ Y
    G = (G + G.T) / 2
    w, Q = np.linalg.eigh(G)
    keep = w > 1e-12 * max(w.max(), 0.0)
    lam = np.zeros(k)
    V = np.zeros((D, k))
    if np.any(keep):
        F = (Y @ Q[:, keep]) / np.sqrt(w[keep])  # C_s ≈ F·Fᵀ (Nyström)
        Qf, R = np.linalg.qr(F)                  # thin SVD of F without forming FᵀF
        Ur, sig, _ = np.linalg.svd(R)
        r = min(k, sig.size)
        lam[:r] = sig[:r] ** 2
        V[:, :r] = Qf @ Ur[:, :r]
    lam_res = max((c.sum() - lam.sum()) / (D - k), 0.0) if D > k else 0.0
    dm = np.maximum(lam - lam_res, 0.0)
    d = np.maximum(c - (V * V) @ dm, 1e-3 * c)
    sh = n / (n + 5.0)                          # Stan's shrinkage, get_estimation (src/adaptation/massmatrix.jl)
    A = s0 * s0 * (sh * d + 1e-3 * (5.0 / (n + 5.0)))
    B = s0[:, None] * V
    st.V = V
    return A, B, np.diag(sh * dm)


def lowrank_fresh_normals(st: LowRankState, ncols):
    """stand-in for the engine's Philox stream (no RNG parity: follow the engine by reading its Ω back)"""
    return np.random.default_rng([st.seed, st.n_fits + 1]).standard_normal((st.mu.size, ncols))


def lowrank_restart(st: LowRankState, fresh=None):
    """start the next window: s₀ ← the window's standard deviations (a coordinate that did not move keeps its s₀), Ω ← [V | fresh
    normals] when the window was fitted — one step of subspace iteration per window —, the sums ← 0"""
    if st.V is not None:
        if st.n >= 2:
            sd = np.sqrt(st.m2 / (st.n - 1))
            st.s0 = np.where(sd > 0, sd, st.s0)
        ncols = st.ell - st.k
        if fresh is None:
            fresh = lowrank_fresh_normals(st, ncols)
        st.Omega = np.concatenate([st.V, np.asarray(fresh, dtype=np.float64).reshape(st.mu.size, ncols)], axis=1)
        st.V = None
    st.n_fits += 1
    st.n = 0
    st.mu = np.zeros_like(st.mu)
    st.m2 = np.zeros_like(st.m2)
    st.Z = np.zeros_like(st.Z)
    return st
