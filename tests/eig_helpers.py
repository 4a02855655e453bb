"""A numpy restatement of the device's dense symmetric eigensolver (pygsp_amd/csrc/gspx_eig.hip.h): two-sided cyclic
block Jacobi with the same block size, round-robin schedule, skip threshold, padding rule and finish.  It is what the
CPU tests hold to the accuracy bars and what the GPU tests compare sweep counts against.  The arithmetic inside a
product differs (numpy's matmul against the matrix cores' summation order), so results agree to rounding, not bits."""
import numpy as np

BLOCK = 32          # JAC_B: a pair of blocks is a 64 x 64 subproblem
INNER_SWEEPS = 2    # JAC_INNER: scalar Jacobi sweeps per subproblem


def round_robin(m, r):
    """The floor(m / 2) disjoint pairs (i < j) of round r (0 <= r < rounds(m)) over m players: the circle method with
    the last of an even field fixed; an odd field plays with one phantom, whose partner has the bye."""
    me = m + (m & 1)
    if me < 2:
        return []
    pairs = []
    for k in range(me // 2):
        a, b = (me - 1, r) if k == 0 else ((r + k) % (me - 1), (r - k) % (me - 1))
        if a < m and b < m:
            pairs.append((min(a, b), max(a, b)))
    return pairs


def rounds(m):
    return (m + 1) // 2 * 2 - 1 if m > 0 else 0


def n_blocks(n):
    return max(2, -(-n // BLOCK)) if n > 0 else 0


def pad_values(gersh, count):
    """Diagonal entries of the padding: distinct, strictly above the Gershgorin bound of A."""
    return (2.0 + np.arange(count)) * max(gersh, 1.0)


def rotation(app, aqq, apq):
    """(c, s) of the Jacobi rotation that zeroes apq, the smaller angle; the identity where apq == 0."""
    safe = np.where(apq == 0, 1.0, apq)
    with np.errstate(over="ignore"):  # (a huge tau gives t = 0: the identity, as on the device)
        tau = (aqq - app) / (2.0 * safe)
        t = np.where(tau >= 0, 1.0, -1.0) / (np.abs(tau) + np.sqrt(1.0 + tau * tau))
    c = 1.0 / np.sqrt(1.0 + t * t)
    s = t * c
    return np.where(apq == 0, 1.0, c), np.where(apq == 0, 0.0, s)


def sub_solve(S, inner=INNER_SWEEPS):
    """Q (m x m, near the identity) of `inner` parallel-order scalar Jacobi sweeps on the symmetric S; S is
    overwritten with Q^T S Q."""
    m = S.shape[0]
    Qt = np.eye(m)
    for _ in range(inner):
        for r in range(rounds(m)):
            pq = np.array(round_robin(m, r))
            p, q = pq[:, 0], pq[:, 1]
            c, s = rotation(S[p, p], S[q, q], S[p, q])
            Sp, Sq = S[:, p].copy(), S[:, q].copy()
            S[:, p], S[:, q] = c * Sp - s * Sq, s * Sp + c * Sq
            Sp, Sq = S[p, :].copy(), S[q, :].copy()
            S[p, :], S[q, :] = c[:, None] * Sp - s[:, None] * Sq, s[:, None] * Sp + c[:, None] * Sq
            S[p, q] = S[q, p] = 0.0
            Qp, Qq = Qt[p, :].copy(), Qt[q, :].copy()
            Qt[p, :], Qt[q, :] = c[:, None] * Qp - s[:, None] * Qq, s[:, None] * Qp + c[:, None] * Qq
    return Qt.T


def off_columns(A):
    """Squared off-diagonal norm of every row of A (summed directly, never as ||A||^2 - sum a_ii^2)."""
    return np.sum(np.square(A - np.diag(np.diag(A))), axis=1)


def sym_eig(A0, tol=1e-13, max_sweeps=30, inner=INNER_SWEEPS):
    """(e ascending, V with the eigenvectors in columns, stats) of the symmetric A0.  ValueError after max_sweeps."""
    A0 = np.array(A0, dtype=np.float64)
    n = A0.shape[0]
    stats = {"sweeps": 0, "rotated": 0, "skipped": 0, "skipped_per_sweep": []}
    if n == 0:
        return np.zeros(0), np.zeros((0, 0)), stats
    nb = n_blocks(n)
    npad = nb * BLOCK
    norm = float(np.sqrt(np.sum(np.square(A0))))
    gersh = float(np.max(np.sum(np.abs(A0), axis=1)))
    A = np.zeros((npad, npad))
    A[:n, :n] = A0
    A[np.arange(n, npad), np.arange(n, npad)] = pad_values(gersh, npad - n)
    V = np.eye(npad)
    while True:
        # stop when off(A) <= tol ||A||_F and no column's off-diagonal part exceeds tol max |a_ii| (its residual)
        col2 = off_columns(A)
        off, worst = float(np.sqrt(np.sum(col2))), float(np.sqrt(np.max(col2)))
        rho = float(np.max(np.abs(np.diag(A)[:n])))
        stats["off_rel"] = off / norm if norm > 0 else 0.0
        if off <= tol * norm and worst <= tol * rho:
            break
        # a pair is skipped below thr: if every pair skips, both criteria hold
        thr2 = (tol * min(norm / nb, rho / np.sqrt(nb))) ** 2
        if stats["sweeps"] >= max_sweeps:
            raise ValueError("sym_eig: no convergence in {} sweeps (off / norm = {:.3e})".format(max_sweeps,
                                                                                                   stats["off_rel"]))
        skipped = 0
        for r in range(rounds(nb)):
            for (bi, bj) in round_robin(nb, r):
                ij = np.r_[bi * BLOCK:(bi + 1) * BLOCK, bj * BLOCK:(bj + 1) * BLOCK]
                S = A[np.ix_(ij, ij)]
                S = (S + S.T) / 2
                if np.sum(np.square(S - np.diag(np.diag(S)))) <= thr2:
                    skipped += 1
                    continue
                Q = sub_solve(S, inner)
                A[:, ij] = A[:, ij] @ Q
                V[:, ij] = V[:, ij] @ Q
                A[ij, :] = Q.T @ A[ij, :]
        stats["sweeps"] += 1
        stats["skipped"] += skipped
        stats["rotated"] += nb * (nb - 1) // 2 - skipped
        stats["skipped_per_sweep"].append(skipped)
    # finish: ascending order of diag(A) (the padding sorts last), one Newton-Schulz step, Rayleigh quotients
    order = np.argsort(np.diag(A), kind="stable")[:n]
    X = V[:n, order]
    stats["pad_mass"] = float(np.max(np.abs(V[n:, order]))) if npad > n else 0.0
    X = X @ (1.5 * np.eye(n) - 0.5 * (X.T @ X))
    W = A0 @ X
    e = np.maximum.accumulate(np.sum(X * W, axis=0))  # (ascending: a cluster's quotients may swap by a rounding error)
    stats["residual"] = float(np.max(np.sqrt(np.sum(np.square(W - X * e[None, :]), axis=0))))
    return e, X, stats


def bars(A, e, U):
    """The three figures the accuracy bars are set on: (max |e - eigvalsh(A)| / s, max |A U - U diag(e)| / s,
    max |U^T U - I|), s = max(lambda_max, 1)."""
    n = A.shape[0]
    if n == 0:
        return 0.0, 0.0, 0.0
    ref = np.linalg.eigvalsh(A)
    s = max(float(ref[-1]), 1.0)
    return (float(np.max(np.abs(e - ref))) / s, float(np.max(np.abs(A @ U - U * e[None, :]))) / s,
            float(np.max(np.abs(U.T @ U - np.eye(n)))))
