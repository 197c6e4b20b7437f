# Test-side restatement of 4-bit product quantization (spec "nbits": 4;
# DESIGN.md §6d), op for op in float32, so the GPU tests can compare D, I
# and the inverted-list bytes bitwise. oracle/ keeps its nbits == 8 assert;
# this class reuses its IVF base, adc_scan, search_preassigned and merge.
#
# ksub = 16; codebooks (m, 16, dsub) fp32; codes kept UNPACKED (n, m) with
# values 0..15. LUT entry (j, c): fp32, t ascending, separate mul and add
# — L2 (r_t - cb_t)^2 on the residual, IP q_t * cb_t with the coarse bias.
# Row distance: acc = 0, acc = acc + lut[j, c_j] for j ascending.
# Packed rows (what the engine stores): byte b = code[2b] | code[2b+1] << 4
# (the faiss ProductQuantizer bit order); odd m leaves the last high
# nibble 0.
import numpy as np

from oracle.core import (METRIC_L2, OracleIVFPQ, _OracleIVFBase, assign_batch,
                         kmeans, seq_ip)

KSUB = 16


def pack(codes):
    """(n, m) codes 0..15 -> (n, (m + 1) // 2) uint8 packed rows."""
    codes = np.asarray(codes)
    assert codes.ndim == 2 and (codes >= 0).all() and (codes < KSUB).all()
    n, m = codes.shape
    c = np.zeros((n, 2 * ((m + 1) // 2)), np.uint8)
    c[:, :m] = codes
    return (c[:, 0::2] | (c[:, 1::2] << 4)).astype(np.uint8)


def unpack(packed, m):
    """(n, >= (m + 1) // 2) packed rows -> (n, m) uint8 codes 0..15."""
    packed = np.asarray(packed, np.uint8)[:, :(m + 1) // 2]
    c = np.empty((packed.shape[0], 2 * packed.shape[1]), np.uint8)
    c[:, 0::2] = packed & 15
    c[:, 1::2] = packed >> 4
    return c[:, :m]


class OraclePQ4(OracleIVFPQ):
    """IndexIVFPQ with 4-bit codes restated: OracleIVFPQ with 16 codewords
    per sub-quantizer."""

    def __init__(self, d, nlist, m, metric, seed=1234):
        # the parent asserts nbits == 8: initialise the IVF base directly
        _OracleIVFBase.__init__(self, d, nlist, metric, seed)
        assert d % m == 0, f"dim {d} not divisible by m={m}"
        self.m = int(m)
        self.dsub = d // m
        self.codebooks = None
        self.lut_f16 = False  # no fp16 tables at 4 bits
        self.list_codes = [np.empty((0, m), dtype=np.uint8)
                           for _ in range(self.nlist)]

    def train(self, x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        self.centroids = kmeans(x, self.nlist, self.metric, self.seed,
                                max_points_per_centroid=self.max_ppc)
        assign = assign_batch(x, self.centroids, self.metric)
        resid = x - self.centroids[assign]
        cb = np.empty((self.m, KSUB, self.dsub), dtype=np.float32)
        for j in range(self.m):
            sub = resid[:, j * self.dsub:(j + 1) * self.dsub]
            cb[j] = kmeans(sub, KSUB, METRIC_L2, self.seed + 1 + j,
                           max_points_per_centroid=self.max_ppc)
        self.codebooks = cb
        self.is_trained = True

    def encode(self, x):
        """(assign, codes): coarse assignment + per-subspace argmin over the
        16 codewords (sequential fp32 distances, lowest index on ties)."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        assign = assign_batch(x, self.centroids, self.metric)
        resid = x - self.centroids[assign]
        codes = np.empty((x.shape[0], self.m), dtype=np.uint8)
        for j in range(self.m):
            sub = resid[:, j * self.dsub:(j + 1) * self.dsub]
            acc = np.zeros((sub.shape[0], KSUB), dtype=np.float32)
            for t in range(self.dsub):
                diff = sub[:, t, None] - self.codebooks[j][None, :, t]
                acc = acc + diff * diff
            codes[:, j] = np.argmin(acc, axis=1).astype(np.uint8)
        return assign, codes

    def build_lut(self, qi, li):
        """(lut (m, 16) fp32, bias) for one (query, probe)."""
        lut = np.empty((self.m, KSUB), dtype=np.float32)
        if self.metric == METRIC_L2:
            r = qi - self.centroids[li]
            for j in range(self.m):
                rs = r[j * self.dsub:(j + 1) * self.dsub]
                acc = np.zeros(KSUB, dtype=np.float32)
                for t in range(self.dsub):
                    diff = np.float32(rs[t]) - self.codebooks[j][:, t]
                    acc = acc + diff * diff
                lut[j] = acc
            return lut, np.float32(0.0)
        for j in range(self.m):
            qs = qi[j * self.dsub:(j + 1) * self.dsub]
            acc = np.zeros(KSUB, dtype=np.float32)
            for t in range(self.dsub):
                acc = acc + np.float32(qs[t]) * self.codebooks[j][:, t]
            lut[j] = acc
        bias = np.float32(seq_ip(qi, self.centroids[li][None, :])[0])
        return lut, bias

    # add, _scan_one (adc_scan over the unpacked codes), decode_ids,
    # search_preassigned and the merge are the parent's.

    def packed_lists(self):
        """(off, ids, packed code bytes) in CSR order."""
        off = np.zeros(self.nlist + 1, np.int64)
        off[1:] = np.cumsum([len(i) for i in self.list_ids])
        return (off, np.concatenate(self.list_ids),
                pack(np.concatenate(self.list_codes)))

    def load_lists(self, off, ids, packed):
        """Take over inverted lists dumped by an engine (packed rows)."""
        codes = unpack(packed, self.m)
        self.list_ids = [np.asarray(ids[off[l]:off[l + 1]], np.int64)
                         for l in range(self.nlist)]
        self.list_codes = [codes[off[l]:off[l + 1]] for l in range(self.nlist)]
        self.ntotal = int(off[-1])
