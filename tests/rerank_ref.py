"""float64 reference and elementwise bound for k-reciprocal re-ranking (csrc/rerank.hip: agrl_re_ranking), restating
oracle/vmgn_oracle.py:re_ranking in two layers, and the seeded cases tests/test_rerank_ref.py (CPU) and tests/test_gpu_rerank.py share.

Discrete layer (``discrete``): decisions, not roundings. D is the joint squared matrix scaled by its column maxima, computed in fp32
exactly as numpy does (square, max and divide are each one correctly rounded fp32 operation, so the kernel's D must be BIT-equal); the
stable neighbour lists (ties -> lower index); half = np.around(k1 / 2) + 1 (half to even); the reciprocal sets, the 2/3 expansion and the
sorted unique sets. It returns per-sample nu = |set|, the support of V, the support of the k2-expanded V, per-query nnz.

Value layer (``values``) on that D and those sets, in float64 (the reference) or in fp32 with numpy's own operations (then the result
is bit for bit oracle.re_ranking's: the check that the discrete layer is restated correctly): w = exp(-D[i, set]), V = w / sum w, the
mean of the k2 nearest rows, t[i][r] = sum over the non-zero columns c of row i of min(V2[i][c], V2[r][c]), jac = 1 - t / (2 - t),
final = jac fl32(1 - lambda) + D fl32(lambda).

Bound, u = 2^-24 (bounds.U32), every count an upper bound on the fp32 roundings of the kernel's chain; all terms of every sum are
positive, so relative errors carry through the sums:
  w       expf: the device library documents 1 ulp, i.e. 2 u relative. This is ASSUMED, not measured.                        2
  V       numerator w (2), the denominator's terms (2) and its nu - 1 additions, one division:                              nu + 4
  V2      k2 == 1: V itself. Otherwise the worst V among the k2 rows, k2 - 1 additions, the division by k2 (counted k2 + 1):
                                                                                                cV2(i) = max_a (nu_a + 4) + k2 + 1
  t       min is monotone: each term carries the larger of its two operands' errors; nnz_i - 1 additions (counted nnz_i):
                                                                                    chain(i, r) = max(cV2(i), cV2(r)) + nnz_i
  jac     t -> 1 - t / (2 - t) has derivative 2 / (2 - t)^2 <= 2 on t <= 1, so t's error enters doubled; 2 - t, the quotient
          (<= 1) and the subtraction (|jac| <= 1) round once each: 3 u absolute
  final   two products and a sum (one fewer if the compiler contracts to an fma): 3 u (|jac| c_jac + D c_org)
      |got - exact| <= u [ chain(i, r) 2 c_jac t  +  3 c_jac + 3 (|jac| c_jac + D c_org) ] (1 + 2^-10)
The first term is handed to bounds.check_rounded as count ``n`` (per element) times magnitude ``mag`` = 2 c_jac t, the rest as its
``slack``; the factor 1 + 2^-10 covers the second-order terms (chain u < 2^-14 at every size used here). Nothing here was tuned on
a kernel's output. Where two samples share no support t is exactly 0 and jac exactly 1: with lambda = 0, final == 1.0 exactly there
and nowhere else (a shared column adds at least exp(-1) / (nu k2) > 1e-4 to t), so the mask is set membership free of any rounding;
with lambda = 1, final == D[:m, m:] bit for bit.

``mut`` names one deliberate defect for the tests that show the bound can tell (never used for a reference).
A plain module (like sta_ref.py): the tests import it. Everything here runs on the CPU."""
import collections
import functools
import math

import numpy as np
import torch

from oracle import vmgn_oracle as O

U32 = 2.0 ** -24
MUTATIONS = ("half_up", "drop_member", "k2_minus_1", "ge_two_thirds", "tie_order")

# name -> m, n, cluster centres, seed, [(k1, k2)], duplicates. N = m + n picks the top-k form (N % 4 == 0: the register form, NV = 2
# above 1024; otherwise radix) and the rows per thread of rr_jaccard (tid + 256 k). The duplicates also run at k2 = 1: with k2 = 3 the three
# nearest samples of a duplicate are duplicates, every duplicate gets the same expanded row and the output is invariant under ANY order
# among them; at k2 = 1 the four samples left out of their own list keep their empty rows (final == 1.0 in their columns) and the order shows.
CASES = collections.OrderedDict([
    ("odd_k1", dict(m=25, n=231, centres=12, seed=11, settings=[(5, 3), (9, 3), (13, 3)])),       # N = 256: half-to-even
    ("k1_limits", dict(m=40, n=500, centres=5, seed=12, settings=[(30, 31), (1, 1), (1, 2)])),    # half = 16 and 1, k2 = k1 + 1
    ("duplicates", dict(m=17, n=239, centres=12, seed=13, settings=[(8, 3), (8, 1)], dup=12)),    # empty sets, tie order
    ("n33", dict(m=1, n=32, centres=4, seed=14, settings=[(6, 2)])),                              # m = 1, one ragged tile
    ("m_gt_n", dict(m=200, n=56, centres=20, seed=15, settings=[(20, 6)])),                       # query block larger than gallery
    ("nv2", dict(m=300, n=788, centres=60, seed=16, settings=[(20, 6), (20, 1)])),                # N = 1088: k up to 4, NV = 2
    ("ragged", dict(m=70, n=601, centres=40, seed=17, settings=[(20, 6)])),                       # N = 671: radix, unaligned rows
])
METRICS = ("euclidean", "cosine")
GRID = [(name, metric, k1, k2) for name, c in CASES.items() for metric in METRICS for (k1, k2) in c["settings"]]


@functools.lru_cache(maxsize=None)
def world(name, metric):
    """Seeded cluster mixture -> (q_g, q_q, g_g) fp32 numpy, read-only. ``dup`` gallery rows and query 5 are one identical vector."""
    c = CASES[name]
    g = torch.Generator().manual_seed(c["seed"])
    cent = torch.randn((c["centres"], 64), generator=g)
    qf = cent[torch.randint(0, c["centres"], (c["m"],), generator=g)] + 0.5 * torch.randn((c["m"], 64), generator=g)
    gf = cent[torch.randint(0, c["centres"], (c["n"],), generator=g)] + 0.5 * torch.randn((c["n"], 64), generator=g)
    if c.get("dup"):
        rows = torch.arange(c["dup"]) * 19 + 7           # spread over the gallery; all of them after the query
        gf[rows] = qf[5]
    fn = O.euclidean_squared if metric == "euclidean" else O.cosine
    out = tuple(np.ascontiguousarray(fn(a, b).numpy(), dtype=np.float32) for a, b in ((qf, gf), (qf, qf), (gf, gf)))
    if c.get("dup"):
        # a matmul does not promise identical bits for identical feature rows: make the duplicates' distance rows and columns
        # bit-identical in the (symmetrised) joint matrix, so every tie among them is exact and the stable order decides
        m = c["m"]
        q_g, q_q, g_g = out
        J = np.block([[np.minimum(q_q, q_q.T), q_g], [q_g.T, np.minimum(g_g, g_g.T)]])
        S = np.concatenate([[5], m + rows.numpy()])
        J[S, :] = J[5, :]
        J[:, S] = J[:, 5][:, None]
        assert np.array_equal(J, J.T)
        out = tuple(np.ascontiguousarray(a) for a in (J[:m, m:], J[:m, :m], J[m:, m:]))
    for a in out:
        a.setflags(write=False)
    return out


def joint_D(q_g, q_q, g_g):
    """re_ranking.py:33-38 in fp32, operation for operation as numpy does it."""
    X = np.square(np.block([[q_q, q_g], [q_g.T, g_g]]).astype(np.float32)).astype(np.float32)
    return np.ascontiguousarray((X / X.max(axis=0)).T.astype(np.float32))


Discrete = collections.namedtuple("Discrete", "rank half sets nu S1 S2 nnz")


def discrete(D, m, k1, k2, mut=None):
    N = D.shape[0]
    if mut == "tie_order":       # ties -> HIGHER index: what an unstable selection may give
        rank = np.lexsort((np.broadcast_to(-np.arange(N), (N, N)), D), axis=1)[:, :k1 + 1]
    else:
        rank = np.argsort(D, axis=1, kind="stable")[:, :k1 + 1]
    half = (int(math.floor(k1 / 2.0 + 0.5)) if mut == "half_up" else int(np.around(k1 / 2.0))) + 1

    def recip(i, k):
        fwd = rank[i, :k]
        return fwd[(rank[fwd, :k] == i).any(axis=1)]

    sets, S1 = [], np.zeros((N, N), dtype=bool)
    for i in range(N):
        base = recip(i, k1 + 1)
        ext = [base]
        for c in base:
            rc = recip(int(c), half)
            inter = len(np.intersect1d(rc, base))
            if (inter >= 2.0 / 3 * len(rc)) if mut == "ge_two_thirds" else (inter > 2.0 / 3 * len(rc)):
                ext.append(rc)
        idx = np.unique(np.concatenate(ext))
        if mut == "drop_member" and i == 0 and len(idx) > 1:
            idx = np.delete(idx, len(idx) // 2)
        sets.append(idx)
        S1[i, idx] = True
    nu = np.array([len(s) for s in sets])
    kk = k2 - 1 if (mut == "k2_minus_1" and k2 > 1) else k2
    S2 = S1 if kk == 1 else np.stack([S1[rank[i, :kk]].any(axis=0) for i in range(N)])
    return Discrete(rank, half, sets, nu, S1, S2, S2[:m].sum(axis=1))


def values(D, disc, m, k2, dt, mut=None):
    """-> (V2 (N,N), t (m,N), jac (m,N)) in ``dt`` (np.float64: the reference; np.float32: numpy's own fp32, as the oracle)."""
    N = D.shape[0]
    V = np.zeros((N, N), dtype=dt)
    for i, idx in enumerate(disc.sets):
        w = np.exp(-D[i, idx].astype(dt))
        V[i, idx] = w / np.sum(w)
    kk = k2 - 1 if (mut == "k2_minus_1" and k2 > 1) else k2
    if kk != 1:
        V = np.stack([V[disc.rank[i, :kk]].mean(axis=0) for i in range(N)]).astype(dt)
    VT = np.ascontiguousarray(V.T)
    t = np.zeros((m, N), dtype=dt)
    for i in range(m):
        for c in np.nonzero(V[i])[0]:                      # ascending columns; a zero row entry adds + 0.0
            t[i] += np.minimum(V[i, c], VT[c])
    jac = (1 - t / (2.0 - t)).astype(dt)
    return V, t, jac


def restated_fp32(q_g, q_q, g_g, k1=20, k2=6, lambda_value=0.3, mut=None):
    """Both layers in fp32: bit for bit oracle.re_ranking (mut None), or a subtly wrong evaluation for the tests of the bound."""
    m = q_g.shape[0]
    D = joint_D(q_g, q_q, g_g)
    disc = discrete(D, m, k1, k2, mut)
    _, _, jac = values(D, disc, m, k2, np.float32, mut)
    final = jac * (1 - lambda_value) + D[:m] * lambda_value
    return final[:, m:]


class Reference(object):
    """The float64 reference of one problem: D, the discrete layer, t and jac; ``final`` / ``bound`` per lambda."""

    def __init__(self, q_g, q_q, g_g, k1, k2):
        self.m, self.n = q_g.shape
        self.k1, self.k2 = k1, k2
        self.D = joint_D(q_g, q_q, g_g)
        self.disc = discrete(self.D, self.m, k1, k2)
        _, self.t, self.jac = values(self.D, self.disc, self.m, k2, np.float64)
        m, d = self.m, self.disc
        cV = d.nu + 4
        cV2 = cV if k2 == 1 else cV[d.rank[:, :k2]].max(axis=1) + k2 + 1
        self.chain = np.maximum(cV2[:m, None], cV2[None, :]) + d.nnz[:, None]          # (m, N)
        S2 = d.S2.astype(np.float32)
        self.no_overlap = (S2[:m] @ S2[m:].T) == 0                                     # (m, n): final == 1.0 at lambda = 0

    @staticmethod
    def coeffs(lam):
        return float(np.float32(1 - lam)), float(np.float32(lam))   # numpy rounds the Python scalars to fp32

    def final(self, lam):
        cj, co = self.coeffs(lam)
        return (self.jac * cj + self.D[:self.m].astype(np.float64) * co)[:, self.m:]

    def bound(self, lam):
        """-> (exact, mag, n, slack) float64 torch tensors (m, n) for bounds.check_rounded(got, exact, mag, n, torch.float32, slack=slack)."""
        m = self.m
        cj, co = self.coeffs(lam)
        grow = 1.0 + 2.0 ** -10
        mag = 2.0 * cj * self.t[:, m:] * grow
        slack = U32 * (3.0 * cj + 3.0 * (np.abs(self.jac[:, m:]) * cj + self.D[:m, m:].astype(np.float64) * co)) * grow
        n = self.chain[:, m:].astype(np.float64)
        return tuple(torch.from_numpy(np.ascontiguousarray(a)) for a in (self.final(lam), mag, n, slack))

    def abs_bound(self, lam):
        _, mag, n, slack = self.bound(lam)
        return (n * U32 * mag + slack).numpy()


@functools.lru_cache(maxsize=None)
def reference(name, metric, k1, k2):
    """Computed once per problem and shared; callers must not write to it."""
    return Reference(*world(name, metric), k1=k1, k2=k2)


def worst_ratio(got, ref, lam):
    """max |got - exact| / bound over the elements (inf for a non-finite output), without asserting or logging."""
    got = np.asarray(got, dtype=np.float64)
    err = np.abs(got - ref.final(lam))
    ratio = np.where(np.isfinite(got), err / np.maximum(ref.abs_bound(lam), 1e-300), np.inf)
    return float(np.where(err == 0, 0.0, ratio).max())


def ranking_outside_near_ties(got, ref, lam, cols=20):
    """Number of positions among the first ``cols`` of the stable ranking of ``got`` (m, n) that differ from the ranking of the exact
    values by more than a near-tie. If every |got - exact| <= b, the p-th smallest of got is within max_row(b) of the p-th smallest
    of exact (order statistics are 1-Lipschitz in the max norm), and got's p-th element g is within b[g] of its own exact value: so
    |exact[e_p] - exact[g_p]| <= max_row(b) + b[g_p] wherever the two rankings name different elements e_p, g_p."""
    exact, b = ref.final(lam), ref.abs_bound(lam)
    cols = min(cols, exact.shape[1])
    og = np.argsort(np.asarray(got), axis=1, kind="stable")[:, :cols]
    oe = np.argsort(exact, axis=1, kind="stable")[:, :cols]
    gap = np.abs(np.take_along_axis(exact, og, 1) - np.take_along_axis(exact, oe, 1))
    tol = b.max(axis=1, keepdims=True) + np.take_along_axis(b, og, 1)
    differ = og != oe
    return int((differ & (gap > tol)).sum()), int(differ.sum())
