# Test-side restatement of the 4- and 6-bit scalar quantizers (spec
# "sq_type": "4bit" | "6bit"), op for op in float32, so the
# GPU tests can compare D, I, reconstructions and the inverted-list bytes
# bitwise. oracle/ keeps its qtype in ("fp16", "8bit") assert; this class
# reuses its IVF base, add, search_preassigned, decode_ids and merge.
#
# B = 4 | 6, Q = (1 << B) - 1. vmin / vdiff per dimension over the training
# residuals (vdiff == 0 -> 1), scale = vdiff / Q in fp32.
# Encode: xi = (r - vmin) / vdiff, c = clamp(int(Q * xi), 0, Q), truncating.
# Decode: vmin + (c + 0.5) * scale (the folded faiss codec, as SQ8).
# Codes are kept UNPACKED (n, d) uint8; pack() gives the stored rows, a
# little-endian bit stream (faiss Codec4bit / Codec6bit):
#   4-bit: byte t // 2 holds dim t in bits 4 * (t & 1);
#   6-bit: dims 4g .. 4g+3 in bytes 3g .. 3g+2, code i at bit 6i of that
#          24-bit little-endian word;
# code_bytes = ceil(d * B / 8), every bit past d * B zero.
# Row distance: the SQ8 folded algebra with cf = float(c): 8 partials, lane
# l summing dims {16l + 128c + b} (c, then b ascending) sequentially, the
# partials combined as ((p0+p4)+(p2+p6)) + ((p1+p5)+(p3+p7)).
import numpy as np

from oracle.core import (METRIC_L2, OracleIVFSQ, _OracleIVFBase, assign_batch,
                         kmeans, seq_ip)


def code_bytes(d, bits):
    return (d * bits + 7) // 8


def stride(d, bits):
    return (code_bytes(d, bits) + 15) // 16 * 16


def pack(codes, bits):
    """(n, d) codes 0 .. 2^bits - 1 -> (n, ceil(d * bits / 8)) uint8 rows."""
    codes = np.asarray(codes)
    assert bits in (4, 6) and codes.ndim == 2
    if (codes < 0).any() or (codes >= (1 << bits)).any():
        raise ValueError(f"code out of range for {bits} bits")
    n, d = codes.shape
    out = np.zeros((n, code_bytes(d, bits)), np.uint8)
    for t in range(d):
        c = codes[:, t].astype(np.uint32)
        bit = t * bits  # position in the row's little-endian bit stream
        by, sh = bit >> 3, bit & 7
        out[:, by] |= ((c << sh) & 0xFF).astype(np.uint8)
        if sh + bits > 8:
            out[:, by + 1] |= (c >> (8 - sh)).astype(np.uint8)
    return out


def unpack(packed, d, bits):
    """(n, >= ceil(d * bits / 8)) packed rows -> (n, d) uint8 codes."""
    packed = np.asarray(packed, np.uint8)
    assert bits in (4, 6) and packed.shape[1] >= code_bytes(d, bits)
    out = np.empty((packed.shape[0], d), np.uint8)
    for t in range(d):
        bit = t * bits
        by, sh = bit >> 3, bit & 7
        w = packed[:, by].astype(np.uint32)
        if sh + bits > 8:
            w = w | (packed[:, by + 1].astype(np.uint32) << 8)
        out[:, t] = (w >> sh) & ((1 << bits) - 1)
    return out


class OracleSQBits(OracleIVFSQ):
    """IndexIVFScalarQuantizer with QT_4bit / QT_6bit restated."""

    def __init__(self, d, nlist, metric, bits, seed=1234):
        # the parent asserts its two qtypes: initialise the IVF base directly
        _OracleIVFBase.__init__(self, d, nlist, metric, seed)
        assert bits in (4, 6)
        self.bits = int(bits)
        self.Q = np.float32((1 << bits) - 1)
        self.qtype = f"{bits}bit"
        self.vmin = self.vdiff = self.scale = None
        self.code_bytes = code_bytes(d, bits)
        self.list_codes = [np.empty((0, d), dtype=np.uint8)
                           for _ in range(self.nlist)]

    def set_ranges(self, vmin, vdiff):
        self.vmin = np.ascontiguousarray(vmin, np.float32)
        self.vdiff = np.ascontiguousarray(vdiff, np.float32)
        self.scale = (self.vdiff / self.Q).astype(np.float32)

    def train(self, x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        self.centroids = kmeans(x, self.nlist, self.metric, self.seed,
                                max_points_per_centroid=self.max_ppc)
        assign = assign_batch(x, self.centroids, self.metric)
        resid = x - self.centroids[assign]
        vmin = resid.min(axis=0).astype(np.float32)
        vdiff = (resid.max(axis=0).astype(np.float32) - vmin).astype(np.float32)
        vdiff[vdiff == 0] = np.float32(1.0)
        self.set_ranges(vmin, vdiff)
        self.is_trained = True

    def _encode_resid(self, resid):
        resid = np.asarray(resid, np.float32)
        xi = (resid - self.vmin[None, :]) / self.vdiff[None, :]
        qi = int(self.Q)
        return np.clip((self.Q * xi).astype(np.int32), 0, qi).astype(np.uint8)

    def _decode_codes(self, codes):
        return self.vmin[None, :] + (
            codes.astype(np.float32) + np.float32(0.5)) * self.scale[None, :]

    # add (unpacked codes through _encode_resid), decode_ids,
    # search_preassigned and the merge are the parent's.

    def _scan_one(self, qi, li, bias):
        codes = self.list_codes[li]
        if codes.shape[0] == 0:
            return None
        cf = codes.astype(np.float32)
        if self.metric == METRIC_L2:
            r = (qi - self.centroids[li]).astype(np.float32)
            u = (r - self.vmin) - np.float32(0.5) * self.scale
            v = self.scale

            def term(t):
                diff = u[t] - cf[:, t] * v[t]
                return diff * diff
        else:
            v = (qi * self.scale).astype(np.float32)
            u = qi * self.vmin + np.float32(0.5) * v

            def term(t):
                return u[t] + cf[:, t] * v[t]

        parts = [np.zeros(codes.shape[0], dtype=np.float32) for _ in range(8)]
        for lane in range(8):
            for t0 in range(lane * 16, self.d, 128):
                for t in range(t0, min(t0 + 16, self.d)):
                    parts[lane] = parts[lane] + term(t)
        acc = ((parts[0] + parts[4]) + (parts[2] + parts[6])) + (
            (parts[1] + parts[5]) + (parts[3] + parts[7]))
        if self.metric == METRIC_L2:
            return acc, self.list_ids[li]
        if bias is None:
            bias = np.float32(seq_ip(qi, self.centroids[li][None, :])[0])
        return bias + acc, self.list_ids[li]

    def packed_lists(self):
        """(off, ids, packed code bytes) in CSR order."""
        off = np.zeros(self.nlist + 1, np.int64)
        off[1:] = np.cumsum([len(i) for i in self.list_ids])
        return (off, np.concatenate(self.list_ids),
                pack(np.concatenate(self.list_codes), self.bits))

    def load_lists(self, off, ids, packed):
        """Take over inverted lists dumped by an engine (packed rows)."""
        codes = unpack(packed, self.d, self.bits)
        self.list_ids = [np.asarray(ids[off[l]:off[l + 1]], np.int64)
                         for l in range(self.nlist)]
        self.list_codes = [codes[off[l]:off[l + 1]] for l in range(self.nlist)]
        self.ntotal = int(off[-1])
