"""Helpers of the SlimQ conversion tests (test_slimq_convert_cpu.py, test_gpu_slimq_convert.py).

quantize_rows_restated is an independent reading of the data-side quantisation of HierarchicalNSWSlimQ::convertFromHNSW, written from
the reference's text (rabitqlib/quantization/rabitq_impl.hpp:38-54 one_bit_code, :75-137 one_bit_code_with_factor,
rabitqlib/utils/space.hpp:272-286 pack_binary) in numpy float32, not from csrc/rabitq_host.hpp.  The reference's reductions
(l2norm_sqr, dot_product) go through Eigen, whose summation order the project does not reproduce; its DEFINITION of them is a strict
left-to-right fp32 sum of rounded products, which is what `chain` does.  Everything else -- the residual, the sign code, xu_cb, the
corner case, the factor expressions -- is the reference's arithmetic in the reference's order, one fp32 rounding per operation.
"""
import numpy as np

F = np.float32
K_CONST_EPSILON = F(1.9)   # rabitqlib/defines.hpp


def chain(terms):
    """((0 + t0) + t1) + ... in fp32."""
    return np.add.accumulate(np.concatenate([np.zeros(1, F), terms.astype(F)]), dtype=F)[-1]


def nearest_centroid_restated(row, cent_raw):
    """The cluster of a row when the caller gives none: the nearest RAW centroid by squared L2, the first minimum."""
    best, cid = np.finfo(F).max, 0
    for c in range(cent_raw.shape[0]):
        t = row - cent_raw[c]
        dd = chain(t * t)
        if dd < best:
            best, cid = dd, c
    return cid


def quantize_row_restated(x, cen, metric):
    """x, cen: rotated row and rotated centroid, float32[padded].  Returns (code uint64[padded / 64], factors float32[3])."""
    dim = x.shape[0]
    with np.errstate(all="ignore"):
        residual = x - cen                                   # one_bit_code :47
        x_u = (residual > 0).astype(np.int32)                # :51
        cb = F(-((1 << 1) - 1) / 2.0)                        # :90
        xu_cb = x_u.astype(F) + cb                           # :92
        l2_sqr = chain(residual * residual)                  # :95
        l2_norm = np.sqrt(l2_sqr)                            # :96
        ip_resi_xucb = chain(residual * xu_cb)               # :99
        ip_cent_xucb = chain(cen * xu_cb)                    # :101
        if ip_resi_xucb == 0:                                # :104-106
            ip_resi_xucb = F(np.inf)
        tmp_error = (l2_norm * K_CONST_EPSILON) * np.sqrt((((l2_sqr * chain(xu_cb * xu_cb)) / (ip_resi_xucb * ip_resi_xucb)) - F(1)) / F(dim - 1))
        if metric == 0:                                      # :124-127
            f_add = l2_sqr + ((F(2) * l2_sqr) * ip_cent_xucb) / ip_resi_xucb
            f_rescale = (F(-2) * l2_sqr) / ip_resi_xucb
            f_error = F(2) * tmp_error
        else:                                                # :128-132
            f_add = (F(1) - chain(residual * cen)) + (l2_sqr * ip_cent_xucb) / ip_resi_xucb
            f_rescale = (-l2_sqr) / ip_resi_xucb
            f_error = F(1) * tmp_error
    code = np.zeros(dim // 64, np.uint64)                    # pack_binary: dimension i -> bit 63 - i % 64 of word i / 64
    for i in np.nonzero(x_u)[0]:
        code[i // 64] |= np.uint64(1) << np.uint64(63 - i % 64)
    return code, np.array([f_add, f_rescale, f_error], F)


def quantize_rows_restated(rows, cent_raw, rotated_rows, rotated_cent, metric, cluster_ids=None):
    n = rows.shape[0]
    cl = np.array([nearest_centroid_restated(rows[i], cent_raw) for i in range(n)], np.uint32) if cluster_ids is None else np.asarray(cluster_ids, np.uint32)
    out = [quantize_row_restated(rotated_rows[i], rotated_cent[cl[i]], metric) for i in range(n)]
    return cl, np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def same_bits_or_nan(got, want):
    """float32 arrays: equal bit patterns, except that where `want` is NaN `got` only has to be a NaN."""
    got, want = np.asarray(got, F), np.asarray(want, F)
    nan = np.isnan(want)
    return got.shape == want.shape and bool(np.all(np.isnan(got[nan]))) and np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))


def clustered_rows(n, d, seed, integer, n_centres=4):
    """Rows around a few centres, each centre itself a row (rows 0 .. n_centres - 1 when n allows): in more than a few dimensions a
    centre is nearer to every row of its cluster than they are to each other, so it collects a reverse edge from most of them -- the
    unions that exceed a level's capacity and go through the re-prune.  integer: small-integer coordinates, so that lists are full of
    equal distances (exact in any summation order)."""
    rng = np.random.default_rng(seed)
    if integer:
        centres = rng.integers(-6, 7, (n_centres, d)).astype(F)
        rows = (centres[rng.integers(0, n_centres, n)] + rng.integers(-2, 3, (n, d))).astype(F)
    else:
        centres = rng.normal(0, 1, (n_centres, d)).astype(F)
        rows = (centres[rng.integers(0, n_centres, n)] + rng.normal(0, 0.35, (n, d))).astype(F)
    if n >= 4 * n_centres:
        rows[:n_centres] = centres
    return rows
