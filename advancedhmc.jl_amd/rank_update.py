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
