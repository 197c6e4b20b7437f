# ORACLE opq — restatement of the OPQ pre-transform (spec "opq": 1; DESIGN.md
# §6f): faiss IndexPreTransform(OPQMatrix(d, M, d2), IndexIVFPQ).
#
#  * OracleOPQ wraps the IVFPQ restatement (core.OracleIVFPQ, 8 or 4 bits)
#    at d_out behind a matrix A
#    (d_out, d_in): y = A x, no bias. The transform itself is computed in
#    float64 and rounded once — exact whenever A is a signed permutation /
#    selection (one non-zero of magnitude 1 per row), which is what the
#    bit-exact GPU tier uses; for a general A it is the fp64 reference of the
#    tolerance tier.
#  * opq_train restates faiss OPQMatrix::train in numpy: centre, seeded
#    Gaussian + QR init, then alternate a plain m x ksub PQ on Y = Xc A^T
#    with the Procrustes update A^T = U V^T of svd(Xc^T Yhat)
#    (numpy.linalg.svd polar factor).
import numpy as np

from .core import METRIC_L2, OracleIVFPQ, assign_batch, kmeans


def transform64(A, x):
    """y = x A^T in float64 (not rounded)."""
    return np.asarray(x, np.float64) @ np.asarray(A, np.float64).T


def transform(A, x):
    """y = x A^T, float64 accumulation, one rounding to float32."""
    return transform64(A, x).astype(np.float32)


def transform_bound(A, x):
    """The project's tolerance tier for y = A x:
    1e-4 * sum_j |A_ij x_j| + 1e-4, per output element."""
    mag = np.abs(np.asarray(x, np.float64)) @ np.abs(np.asarray(A, np.float64)).T
    return 1e-4 * mag + 1e-4


def signed_selection(d_in, d_out, rng):
    """(d_out, d_in) float32: row o has a single +-1 at a distinct column —
    a signed permutation when d_out == d_in. y = A x is exact in any
    summation order."""
    cols = rng.permutation(d_in)[:d_out]
    A = np.zeros((d_out, d_in), np.float32)
    A[np.arange(d_out), cols] = rng.choice(np.float32([-1.0, 1.0]), d_out)
    return A


def random_rotation(d_in, d_out, rng):
    """d_out orthonormal rows of a numpy-QR rotation, float32."""
    q, _ = np.linalg.qr(rng.standard_normal((d_in, d_in)))
    return np.ascontiguousarray(q.T[:d_out]).astype(np.float32)


class OracleOPQ:
    """The inner IVFPQ restatement at d_out behind A."""

    def __init__(self, A, nlist, m, metric, nbits=8, seed=1234):
        self.A = np.ascontiguousarray(A, np.float32)
        self.d_out, self.d_in = self.A.shape
        self.inner = OracleIVFPQ(self.d_out, nlist, m, metric, nbits, seed)
        self.nbits = nbits

    def set_trained(self, centroids, codebooks):
        self.inner.centroids = np.ascontiguousarray(centroids, np.float32)
        self.inner.codebooks = np.ascontiguousarray(codebooks, np.float32)
        self.inner.is_trained = True

    def apply(self, x):
        return transform(self.A, x)

    def add(self, x):
        self.inner.add(self.apply(x))

    def search_preassigned(self, q, probes, keys, k):
        return self.inner.search_preassigned(self.apply(q), probes, keys, k)

    def reconstruct(self, I):
        """(.., d_in) float64: A^T . decode (reverse_transform of an
        orthonormal matrix)."""
        dec = self.inner.decode_ids(I).astype(np.float64)
        return dec @ self.A.astype(np.float64)

    def lists(self):
        """(off, ids, code bytes per row as the engine packs them)."""
        return self.inner.packed_lists()


# ---------------------------------------------------------------------------
# plain PQ (non-residual) and the OPQ trainer
# ---------------------------------------------------------------------------


def _lloyd(x, cent, niter):
    """Hot-started Lloyd iterations (mean update; an empty cluster keeps its
    centroid)."""
    cent = cent.copy()
    for _ in range(niter):
        a = assign_batch(x, cent, METRIC_L2)
        sums = np.zeros(cent.shape, np.float64)
        np.add.at(sums, a, x.astype(np.float64))
        cnt = np.bincount(a, minlength=cent.shape[0])
        nz = cnt > 0
        cent[nz] = (sums[nz] / cnt[nz, None]).astype(np.float32)
    return cent


def pq_train(y, m, ksub, seed=1234, hot=None, niter=25):
    """(m, ksub, dsub) codebooks of a plain PQ on y."""
    y = np.ascontiguousarray(y, np.float32)
    dsub = y.shape[1] // m
    cb = np.empty((m, ksub, dsub), np.float32)
    for j in range(m):
        sub = np.ascontiguousarray(y[:, j * dsub:(j + 1) * dsub])
        if hot is None:
            cb[j] = kmeans(sub, ksub, METRIC_L2, seed + 1000 + j, niter=niter)
        else:
            cb[j] = _lloyd(sub, hot[j], niter)
    return cb


def pq_quantize(y, cb):
    """Encode + decode: the nearest codeword per sub-space."""
    y = np.ascontiguousarray(y, np.float32)
    m, _, dsub = cb.shape
    out = np.empty_like(y)
    for j in range(m):
        sub = np.ascontiguousarray(y[:, j * dsub:(j + 1) * dsub])
        out[:, j * dsub:(j + 1) * dsub] = cb[j][assign_batch(sub, cb[j], METRIC_L2)]
    return out


def pq_mse(y, m, ksub, seed=1234):
    """Mean over rows of |y - PQ(y)|^2 for a PQ trained on y itself."""
    yh = pq_quantize(y, pq_train(y, m, ksub, seed))
    return float(((y.astype(np.float64) - yh) ** 2).sum(axis=1).mean())


def polar_svd(M):
    """Orthonormal polar factor U V^T of the thin SVD of M."""
    u, _, vt = np.linalg.svd(np.asarray(M, np.float64), full_matrices=False)
    return u @ vt


def opq_train(x, m, ksub, d_out=None, niter=8, seed=1234):
    """faiss OPQMatrix::train restated. Returns A (d_out, d_in) float64
    (callers round to float32)."""
    x = np.asarray(x, np.float32)
    d_in = x.shape[1]
    d_out = d_in if d_out is None else d_out
    xc = (x.astype(np.float64) - x.astype(np.float64).mean(axis=0)).astype(np.float32)
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((d_in, d_in)))
    P = q[:, :d_out]  # A^T: (d_in, d_out), orthonormal columns
    cb = None
    for it in range(niter):
        y = (xc.astype(np.float64) @ P).astype(np.float32)
        cb = pq_train(y, m, ksub, seed, hot=cb, niter=25 if it == 0 else 4)
        yh = pq_quantize(y, cb)
        P = polar_svd(xc.astype(np.float64).T @ yh.astype(np.float64))
    return P.T


def recipe(zero_col=None):
    """The structured training input of the OPQ tests: 8 latent factors of
    decaying scale mixed into 32 dims, plus noise."""
    rng = np.random.default_rng(0)
    z = rng.standard_normal((4096, 8)) * np.linspace(3, .5, 8)
    B = rng.standard_normal((8, 32))
    x = (z @ B + .05 * rng.standard_normal((4096, 32))).astype(np.float32)
    if zero_col is not None:
        x[:, zero_col] = 0.0
    return x


def centred(x):
    x64 = np.asarray(x, np.float64)
    return (x64 - x64.mean(axis=0)).astype(np.float32)


def ortho_dev(A):
    """max |A A^T - I| in float64."""
    A = np.asarray(A, np.float64)
    return float(np.abs(A @ A.T - np.eye(A.shape[0])).max())
