# Oracle self-consistency: size-independent properties of the restated
# faiss semantics (SURVEY.md §8c — for IVF numerics the reference ships no
# golden vectors, so the oracle is pinned by properties + our own frozen
# fixtures in tests/golden/).
import numpy as np
import pytest

from oracle import (
    METRIC_INNER_PRODUCT as IP,
    METRIC_L2 as L2,
    OracleFlat,
    OracleIVFFlat,
    OracleIVFPQ,
    OracleIVFSQ,
    kmeans,
    make_oracle_engine,
    save_oracle_engine,
    load_oracle_engine,
    splitmix64_seq,
    partial_shuffle_indices,
)
from oracle.core import FLT_MAX, adc_scan, seq_l2, seq_ip, pairwise_scores


def _data(n, d, seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, d), dtype=np.float32)


def brute_topk(q, xb, k, metric):
    sc = pairwise_scores(q, xb, metric)
    key = sc if metric == L2 else -sc
    ids = np.arange(xb.shape[0])
    out_i = np.stack([np.lexsort((ids, key[i]))[:k] for i in range(q.shape[0])])
    rows = np.arange(q.shape[0])[:, None]
    return sc[rows, out_i], out_i.astype(np.int64)


def test_splitmix64_known_answers():
    # splitmix64 reference values for seed 1234567 (published test vectors
    # of Vigna's splitmix64.c): first three outputs
    out = splitmix64_seq(1234567, 3)
    assert out[0] == np.uint64(6457827717110365317)
    assert out[1] == np.uint64(3203168211198807973)
    assert out[2] == np.uint64(9817491932198370423)


def test_partial_shuffle_deterministic():
    a = partial_shuffle_indices(1000, 10, 42)
    b = partial_shuffle_indices(1000, 10, 42)
    c = partial_shuffle_indices(1000, 10, 43)
    np.testing.assert_array_equal(a, b)
    assert not np.array_equal(a, c)
    assert len(set(a.tolist())) == 10


@pytest.mark.parametrize("metric", [IP, L2])
def test_flat_matches_brute(metric):
    xb = _data(500, 32)
    q = _data(7, 32, seed=1)
    idx = OracleFlat(32, metric)
    idx.add(xb[:300])
    idx.add(xb[300:])
    D, I = idx.search(q, 5)
    Dg, Ig = brute_topk(q, xb, 5, metric)
    np.testing.assert_array_equal(I, Ig)
    np.testing.assert_allclose(D, Dg, rtol=1e-6, atol=1e-5)


def test_flat_padding_when_k_exceeds_ntotal():
    idx = OracleFlat(8, L2)
    idx.add(_data(3, 8))
    D, I = idx.search(_data(2, 8, seed=1), 5)
    assert (I[:, 3:] == -1).all()
    assert (D[:, 3:] == FLT_MAX).all()
    idx_ip = OracleFlat(8, IP)
    idx_ip.add(_data(3, 8))
    D, I = idx_ip.search(_data(2, 8, seed=1), 5)
    assert (I[:, 3:] == -1).all()
    assert (D[:, 3:] == -FLT_MAX).all()


def test_empty_flat_search():
    idx = OracleFlat(8, L2)
    D, I = idx.search(_data(2, 8), 3)
    assert (I == -1).all()


def test_kmeans_deterministic_and_shapes():
    x = _data(2000, 16)
    c1 = kmeans(x, 8, L2, seed=99)
    c2 = kmeans(x, 8, L2, seed=99)
    np.testing.assert_array_equal(c1, c2)
    assert c1.shape == (8, 16)
    # objective sanity: kmeans centroids beat random centroids
    from oracle.core import assign_batch

    a = assign_batch(x, c1, L2)
    obj = ((x - c1[a]) ** 2).sum()
    crand = x[:8]
    ar = assign_batch(x, crand, L2)
    obj_rand = ((x - crand[ar]) ** 2).sum()
    assert obj < obj_rand


@pytest.mark.parametrize("metric", [IP, L2])
def test_ivfflat_full_probe_equals_flat(metric):
    # nprobe == nlist scans everything -> identical ids to exact brute force
    xb = _data(800, 24)
    q = _data(5, 24, seed=3)
    idx = OracleIVFFlat(24, 8, metric, seed=5)
    idx.train(xb[:400])
    idx.add(xb)
    idx.nprobe = 8
    D, I = idx.search(q, 10)
    Dg, Ig = brute_topk(q, xb, 10, metric)
    np.testing.assert_array_equal(I, Ig)
    np.testing.assert_allclose(D, Dg, rtol=1e-4, atol=1e-4)


def test_ivfflat_partial_probe_subset():
    xb = _data(800, 24)
    q = _data(5, 24, seed=3)
    idx = OracleIVFFlat(24, 8, L2, seed=5)
    idx.train(xb[:400])
    idx.add(xb)
    idx.nprobe = 2
    D2, I2 = idx.search(q, 10)
    idx.nprobe = 8
    D8, I8 = idx.search(q, 10)
    # partial-probe results are a (weakly worse) subset of full-probe space
    assert (D2[:, 0] >= D8[:, 0] - 1e-6).all()


def test_ivfpq_identity_on_codebook_points():
    # a vector equal to (centroid + codebook entries) must PQ-scan to ~0 distance
    d, m, nlist = 16, 4, 4
    xb = _data(600, d)
    idx = OracleIVFPQ(d, nlist, m, L2, seed=11)
    idx.train(xb)
    idx.add(xb[:200])
    idx.nprobe = nlist
    # take stored code 0 of list with data and reconstruct it
    li = next(l for l in range(nlist) if idx.list_codes[l].shape[0] > 0)
    code = idx.list_codes[li][0]
    gid = idx.list_ids[li][0]
    rec = idx.centroids[li] + np.concatenate(
        [idx.codebooks[j][code[j]] for j in range(m)]
    )
    D, I = idx.search(rec[None, :], 1)
    assert I[0, 0] == gid
    assert D[0, 0] < 1e-3


def test_adc_scan_equals_decoded_distance():
    # ADC LUT-sum distance == distance to decoded vector (within fp error)
    d, m = 16, 4
    rng = np.random.default_rng(0)
    cb = rng.standard_normal((m, 256, d // m)).astype(np.float32)
    codes = rng.integers(0, 256, size=(50, m)).astype(np.uint8)
    r = rng.standard_normal(d).astype(np.float32)
    lut = np.empty((m, 256), dtype=np.float32)
    for j in range(m):
        rs = r[j * (d // m) : (j + 1) * (d // m)]
        lut[j] = ((rs[None, :] - cb[j]) ** 2).sum(axis=1)
    dist = adc_scan(lut, codes)
    dec = np.concatenate([cb[j][codes[:, j]] for j in range(m)], axis=1)
    ref = ((r[None, :] - dec) ** 2).sum(axis=1)
    np.testing.assert_allclose(dist, ref, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("metric", [IP, L2])
def test_ivfpq_beats_random_ranking(metric):
    # PQ search with full probe must approximate exact ranking: recall@10
    # of exact top-1 should be high on separable data
    d, m = 32, 8
    rng = np.random.default_rng(2)
    centers = rng.standard_normal((16, d)).astype(np.float32) * 5
    pts = centers[rng.integers(0, 16, 2000)] + rng.standard_normal((2000, d)).astype(np.float32) * 0.3
    q = pts[:20] + 0.01 * rng.standard_normal((20, d)).astype(np.float32)
    idx = OracleIVFPQ(d, 8, m, metric, seed=3)
    idx.train(pts)
    idx.add(pts)
    idx.nprobe = 8
    D, I = idx.search(q, 10)
    _, Ig = brute_topk(q, pts, 1, metric)
    hits = sum(1 for i in range(20) if Ig[i, 0] in I[i])
    # IP top-1 is norm-dominated, residual-PQ recall is inherently lower there
    assert hits >= (18 if metric == L2 else 12)


def test_ivfsq8_roundtrip_idempotent():
    d = 16
    idx = OracleIVFSQ(d, 4, L2, qtype="8bit", seed=7)
    xb = _data(500, d)
    idx.train(xb)
    resid = _data(30, d, seed=9) * 0.5
    codes = idx._encode_resid(resid)
    dec = idx._decode_codes(codes)
    codes2 = idx._encode_resid(dec.astype(np.float32))
    np.testing.assert_array_equal(codes, codes2)  # encode∘decode idempotent
    # quantization error bounded by one step
    step = idx.vdiff / 255.0
    assert (np.abs(dec - np.clip(resid, idx.vmin, idx.vmin + idx.vdiff)) <= step + 1e-6).all()


@pytest.mark.parametrize("qtype", ["fp16", "8bit"])
@pytest.mark.parametrize("metric", [IP, L2])
def test_ivfsq_full_probe_close_to_flat(qtype, metric):
    xb = _data(600, 24)
    q = _data(5, 24, seed=3)
    idx = OracleIVFSQ(24, 4, metric, qtype=qtype, seed=5)
    idx.train(xb)
    idx.add(xb)
    idx.nprobe = 4
    D, I = idx.search(q, 5)
    Dg, Ig = brute_topk(q, xb, 5, metric)
    # quantized: top-1 id agrees on well-separated data most of the time;
    # distances close
    agree = (I[:, 0] == Ig[:, 0]).mean()
    assert agree >= 0.8
    np.testing.assert_allclose(D[:, 0], Dg[:, 0], rtol=0.05, atol=0.05)


def test_save_load_roundtrip(tmp_path):
    for spec in [
        {"type": "flat", "dim": 16, "metric": IP},
        {"type": "ivf_flat", "dim": 16, "metric": L2, "nlist": 4, "nprobe": 2},
        {"type": "ivfpq", "dim": 16, "metric": L2, "nlist": 4, "m": 4, "nprobe": 4},
        {"type": "ivfsq", "dim": 16, "metric": IP, "nlist": 4, "sq_type": "8bit", "nprobe": 4},
    ]:
        eng = make_oracle_engine(spec)
        xb = _data(400, 16)
        eng.train(xb)
        eng.add(xb)
        p = str(tmp_path / f"{spec['type']}.dfann")
        save_oracle_engine(eng, p)
        eng2 = load_oracle_engine(p)
        q = _data(3, 16, seed=4)
        D1, I1 = eng.search(q, 5)
        D2, I2 = eng2.search(q, 5)
        np.testing.assert_array_equal(I1, I2)
        np.testing.assert_array_equal(D1, D2)
        assert eng2.ntotal == eng.ntotal


def test_search_and_reconstruct_shapes():
    eng = make_oracle_engine({"type": "ivfpq", "dim": 16, "metric": L2,
                              "nlist": 4, "m": 4, "nprobe": 4})
    xb = _data(400, 16)
    eng.train(xb)
    eng.add(xb)
    q = _data(3, 16, seed=4)
    D, I, R = eng.search_and_reconstruct(q, 5)
    assert R.shape == (3, 5, 16)
    # reconstruction of the top hit is close to the true vector
    err = np.linalg.norm(R[0, 0] - xb[I[0, 0]]) / np.linalg.norm(xb[I[0, 0]])
    assert err < 0.7


# ---------------------------------------------------------------------------
# fp16-LUT option (spec "pq_lut_f16"): half-rounded ADC tables, fp32 sum
# ---------------------------------------------------------------------------


def _pq_pair(metric, d=12, m=4, nlist=3, n=90, seed=70):
    """Exact and fp16-LUT oracle IVFPQ over the same artifacts and rows."""
    rng = np.random.default_rng(seed)
    cent = (rng.standard_normal((nlist, d)) * 4.0).astype(np.float32)
    cb = rng.standard_normal((m, 256, d // m)).astype(np.float32)
    xb = (cent[rng.integers(0, nlist, n)]
          + rng.standard_normal((n, d))).astype(np.float32)
    q = (cent[rng.integers(0, nlist, 5)]
         + rng.standard_normal((5, d))).astype(np.float32)
    out = []
    for f16 in (0, 1):
        spec = {"type": "ivfpq", "dim": d, "metric": metric, "nlist": nlist,
                "m": m, "nprobe": nlist, "pq_lut_f16": f16}
        orc = make_oracle_engine(spec)
        assert orc.lut_f16 == bool(f16)
        orc.centroids, orc.codebooks, orc.is_trained = cent, cb, True
        orc.add(xb)
        out.append(orc)
    return out[0], out[1], q


@pytest.mark.parametrize("metric", [IP, L2])
def test_pq_lut_f16_distance_bound(metric):
    # each of the m summed table entries moves by at most half a half-ulp,
    # i.e. |entry| * 2^-11, so a distance moves by at most
    # m * max|lut| * 2^-11 (the fp32 sums' own rounding is orders below)
    exact, half, q = _pq_pair(metric)
    for qi in q:
        for li in range(exact.nlist):
            lut, _ = exact.build_lut(qi, li)
            assert np.abs(lut).max() < 32752  # half range: no overflow
            de, ids_e = exact._scan_one(qi, li, None)
            dh, ids_h = half._scan_one(qi, li, None)
            np.testing.assert_array_equal(ids_e, ids_h)
            bound = exact.m * float(np.abs(lut).max()) * 2.0 ** -11
            assert np.abs(de.astype(np.float64) - dh).max() <= bound
    # the option changes values: not a no-op
    De, _ = exact.search(q, 10)
    Dh, _ = half.search(q, 10)
    assert not np.array_equal(De, Dh)


@pytest.mark.parametrize("metric", [IP, L2])
def test_pq_lut_f16_hand_restatement(metric):
    # 2 subspaces restated by hand: table entry (sequential t, fp32) ->
    # half -> fp32, then acc = (0 + e0) + e1 in fp32, IP bias added in
    # fp32 in front. Must equal the option's output BITWISE.
    exact, half, q = _pq_pair(metric, d=6, m=2, nlist=2, n=40, seed=71)
    cb, dsub = half.codebooks, 3
    for qi in q:
        for li in range(2):
            codes = half.list_codes[li]
            got, _ = half._scan_one(qi, li, None)
            want = np.empty(codes.shape[0], np.float32)
            for r, code in enumerate(codes):
                acc = np.float32(0.0)
                for j in range(2):
                    e = np.float32(0.0)
                    for t in range(dsub):
                        w = cb[j][code[j]][t]
                        if metric == L2:
                            diff = np.float32(
                                np.float32(qi[j * dsub + t]
                                           - half.centroids[li][j * dsub + t])
                                - w)
                            e = np.float32(e + np.float32(diff * diff))
                        else:
                            e = np.float32(
                                e + np.float32(qi[j * dsub + t] * w))
                    acc = np.float32(acc + np.float32(np.float16(e)))
                if metric == IP:
                    bias = np.float32(0.0)
                    for t in range(6):
                        bias = np.float32(
                            bias + np.float32(qi[t] * half.centroids[li][t]))
                    acc = np.float32(bias + acc)
                want[r] = acc
            np.testing.assert_array_equal(got, want)


def test_pq_lut_f16_half_subnormal_is_gradual():
    # an entry below the smallest normal half (2^-14) keeps its leading
    # bits (gradual underflow), it is not flushed to zero
    v = np.array([2.0 ** -16 * 1.5, 2.0 ** -24, 2.0 ** -26], np.float32)
    h = v.astype(np.float16).astype(np.float32)
    np.testing.assert_array_equal(
        h, np.array([2.0 ** -16 * 1.5, 2.0 ** -24, 0.0], np.float32))


def test_kmeans_reports_empty_splits():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((200, 4)).astype(np.float32)
    st = {}
    kmeans(x, 4, L2, seed=1, stats=st)
    assert st["empty_splits"] == 0
    # 3 distinct points, 5 centroids: some cluster is empty every iteration
    y = np.repeat(np.eye(3, 4, dtype=np.float32), 4, axis=0)
    kmeans(y, 5, L2, seed=1, stats=st)
    assert st["empty_splits"] > 0


def test_spec_max_ppc_caps_the_kmeans_subsample():
    # spec "max_ppc" (the engine's k-means subsample cap per centroid):
    # 400 rows, 4 lists, cap 4*16 = 64 -> training sees the strided 64
    x = _data(400, 6, seed=9)
    spec = {"type": "ivfsq", "dim": 6, "metric": L2, "nlist": 4,
            "sq_type": "8bit", "seed": 5, "max_ppc": 16}
    orc = make_oracle_engine(spec)
    assert orc.max_ppc == 16
    orc.train(x)
    sel = (np.arange(64) * 400) // 64
    np.testing.assert_array_equal(
        orc.centroids, kmeans(x[sel], 4, L2, 5))
    np.testing.assert_array_equal(
        orc.centroids, kmeans(x, 4, L2, 5, max_points_per_centroid=16))
    dflt = make_oracle_engine({k: v for k, v in spec.items() if k != "max_ppc"})
    assert dflt.max_ppc == 256
    dflt.train(x)
    assert not np.array_equal(dflt.centroids, orc.centroids)
    # PQ codebooks train under the same cap, as in the engine
    y = _data(600, 4, seed=10)
    pq = make_oracle_engine({"type": "ivfpq", "dim": 4, "metric": L2,
                             "nlist": 2, "m": 2, "seed": 5, "max_ppc": 2})
    pq.train(y)
    resid = y - pq.centroids[
        np.argmin(pairwise_scores(y, pq.centroids, L2), axis=1)]
    np.testing.assert_array_equal(
        pq.codebooks[1],
        kmeans(resid[:, 2:], 256, L2, 5 + 1 + 1, max_points_per_centroid=2))
