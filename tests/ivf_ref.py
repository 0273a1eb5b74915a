"""IVF index: file parser, float64 reference and DERIVED error bounds (plain NumPy, no GPU).  TEST INFRASTRUCTURE.

The index file (ivfpq_io.hip) holds every device array of an index, so a test can build on the GPU, save, parse the
file here and check each array against what the documented contract says it must be, computed in float64 from the
corpus rows.  Nothing in this module mirrors a kernel's instruction order: the references are the plain formulas of
ivfpq.h's header comment, and every tolerance is a forward error bound of the number format the kernel computes in.

Bounds.  u = 2^-24 is f32's unit roundoff and gamma_n = n u / (1 - n u) the classic bound of n chained roundings
(Higham, Accuracy and Stability of Numerical Algorithms, ch. 3): an n-term f32 dot product summed in ANY order is off
by at most gamma_n * sum |a_i b_i|.  The MFMA and wave-reduction orders of the kernels are all covered by "any order".
"""
import struct

import numpy as np

DIM = 256
PQ_M, PQ_K, PQ_DSUB = 32, 256, 8
LP_DIMS = 32
MAGIC = b"SMTIVFP1"
U32 = 2.0 ** -24          # unit roundoff of f32 (round to nearest)


def gamma(n, u=U32):
    return n * u / (1.0 - n * u)


# ---------------------------------------------------------------------------------------------- file format
def index_file_size(nlist, n_rows, kind):
    size = 64 + nlist * DIM * 4 + nlist * 4 + PQ_M * PQ_K * PQ_DSUB * 4 + (nlist + 1) * 8 + n_rows * 4 + n_rows * PQ_M
    if kind == 1:
        size += nlist * LP_DIMS * DIM * 4 + nlist * LP_DIMS * 4
    return size


def read_index(path):
    """The arrays of a saved index as a dict: nlist, n_rows, kind, centroids [nlist][256] f32, cnorm_half [nlist] f32,
    codebooks [32][256][8] f32, offsets [nlist+1] u64, ids [N] u32, codes [N][32] u8 and, for kind 1, basis [nlist][32][256]
    f32 and lscale [nlist][32] f32.  Raises ValueError on a wrong magic, an unsupported geometry or a file whose size is not
    exactly what its header implies."""
    with open(path, "rb") as f:
        blob = f.read()
    if len(blob) < 64 or blob[:8] != MAGIC:
        raise ValueError(f"{path}: not an IVF index file")
    nlist, m, nbits, dim, n_rows = struct.unpack_from("<IIIIQ", blob, 8)
    refine, kind = blob[32], blob[33]
    if m != PQ_M or nbits != 8 or dim != DIM or nlist < 32 or nlist > 4096 or nlist % 32 or kind > 1 or refine != 0:
        raise ValueError(f"{path}: unsupported geometry (nlist {nlist}, m {m}, nbits {nbits}, dim {dim}, kind {kind})")
    if any(blob[34:64]):
        raise ValueError(f"{path}: non-zero padding in the header")
    if len(blob) != index_file_size(nlist, n_rows, kind):
        raise ValueError(f"{path}: {len(blob)} bytes, the header implies {index_file_size(nlist, n_rows, kind)}")
    pos = [64]

    def take(dtype, *shape):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        a = np.frombuffer(blob, dtype=dtype, count=int(np.prod(shape)), offset=pos[0]).reshape(shape)
        pos[0] += n
        return a

    ix = dict(nlist=nlist, n_rows=n_rows, kind=kind)
    ix["centroids"] = take("<f4", nlist, DIM)
    ix["cnorm_half"] = take("<f4", nlist)
    ix["codebooks"] = take("<f4", PQ_M, PQ_K, PQ_DSUB)
    ix["offsets"] = take("<u8", nlist + 1)
    ix["ids"] = take("<u4", n_rows)
    ix["codes"] = take("u1", n_rows, PQ_M)
    if kind == 1:
        ix["basis"] = take("<f4", nlist, LP_DIMS, DIM)
        ix["lscale"] = take("<f4", nlist, LP_DIMS)
    assert pos[0] == len(blob)
    return ix


def write_index(path, ix):
    """The inverse of read_index (the CPU tests build an index in NumPy and write it in the file format)."""
    head = MAGIC + struct.pack("<IIIIQ", ix["nlist"], PQ_M, 8, DIM, ix["n_rows"]) + bytes([0, ix["kind"]]) + bytes(30)
    assert len(head) == 64
    parts = [head, ix["centroids"].astype("<f4").tobytes(), ix["cnorm_half"].astype("<f4").tobytes(),
             ix["codebooks"].astype("<f4").tobytes(), ix["offsets"].astype("<u8").tobytes(), ix["ids"].astype("<u4").tobytes(),
             ix["codes"].astype("u1").tobytes()]
    if ix["kind"] == 1:
        parts += [ix["basis"].astype("<f4").tobytes(), ix["lscale"].astype("<f4").tobytes()]
    with open(path, "wb") as f:
        f.write(b"".join(parts))


def list_of_rows(ix):
    """list_of[row] = the list the row sits in, pos_of[row] = its position in list order."""
    sizes = np.diff(ix["offsets"].astype(np.int64))
    list_of_pos = np.repeat(np.arange(ix["nlist"]), sizes)
    list_of = np.empty(ix["n_rows"], dtype=np.int64)
    list_of[ix["ids"]] = list_of_pos
    pos_of = np.empty(ix["n_rows"], dtype=np.int64)
    pos_of[ix["ids"]] = np.arange(ix["n_rows"])
    return list_of, pos_of


# ---------------------------------------------------------------------------------------------- bounds
def dot_bound(a, b, n=None, u=U32):
    """Forward error bound of an f32 dot product over the last axis: gamma_n * sum |a_i b_i| (n = its length: 256 for rows)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    n = a.shape[-1] if n is None else n
    return gamma(n, u) * np.sum(np.abs(a * b), axis=-1)


def pair_abs(x, c):
    """sum_i |x_i c_i| for every (row, centroid) pair: what dot_bound scales, as one matrix product."""
    return np.abs(np.asarray(x, dtype=np.float64)) @ np.abs(np.asarray(c, dtype=np.float64)).T


# The build's assignment (ivf_assign_kernel) forms x . c from bf16 x 3 split products by default (tuning key gemm_bf16x3 = 1;
# mfma_tile.h), NOT from f32 products, so its bound takes its constants from bf16:
#   representation: x = xh + xl + ex with |xl| <= 2^-8 |x|, |ex| <= 2^-16 |x| (two roundings to 8 significant bits), likewise c;
#     computed is xh.ch + xl.ch + xh.cl, dropped is xl.cl + ex.c + (xh + xl).ec, each term <= 2^-16 (1 + 2^-16) sum |x_i c_i|;
#   accumulation: 16 K-steps x 3 instructions x 16 products = 768 exact products (8 x 8 significant bits fit f32) added into one
#     f32 accumulator: gamma_768 * sum |terms| in any order, sum |terms| <= (1 + 2^-8)(1 + 2^-7) sum |x_i c_i|.  (This takes an
#     MFMA's internal 16-term sum to be no worse than 16 separately rounded f32 additions; the project measured <= 2 ulp per
#     instruction, well inside that.)
BF16X3_COEF = 3 * 2.0 ** -16 * (1 + 2.0 ** -15) + gamma(768) * (1 + 2.0 ** -6)
F32_COEF = gamma(DIM)


def score_bound(abs_xc, dot, cnh, coef):
    """Bound on |computed - exact| of the assignment / probe score x.c - 0.5|c|^2:  coef * sum|x_i c_i| for the dot product, the SAME
    f32 bound gamma_256 on the 256 squares behind 0.5|c|^2 (cnorm_half_kernel), and one f32 rounding of the subtraction (2u covers
    the rounding of the difference of two already rounded values to first order and beyond)."""
    return coef * abs_xc + gamma(DIM) * np.abs(cnh) + 2 * U32 * (np.abs(dot) + np.abs(cnh))


# ivf_unit_queries_kernel brings a query to unit length in f32: 256 squares summed (relative gamma_256 -- all terms positive),
# a reciprocal square root (halves the relative error; <= 2u of its own) and one multiply per component (u): every component of the
# f32 unit query is within gamma_260 of the float64 one, RELATIVE, so q^.c moves by at most gamma_260 * sum |q^_i c_i|.
UNIT_QUERY_COEF = gamma(260)


# ---------------------------------------------------------------------------------------------- reference functions
def assign_scores(x, centroids):
    """x.c - 0.5|c|^2 in float64 for every (row, centroid) pair: its arg-max is the nearest centroid."""
    x, c = np.asarray(x, dtype=np.float64), np.asarray(centroids, dtype=np.float64)
    return x @ c.T - 0.5 * np.sum(c * c, axis=1)[None, :]


def pq_nearest(residual, codebooks):
    """float64 squared distances of every residual sub-vector to all 256 codewords of its subspace: [n][32][256]."""
    r = np.asarray(residual, dtype=np.float64).reshape(-1, PQ_M, PQ_DSUB)
    cb = np.asarray(codebooks, dtype=np.float64)
    out = np.empty((r.shape[0], PQ_M, PQ_K))
    for s in range(PQ_M):
        t = r[:, s, None, :] - cb[s][None, :, :]
        out[:, s, :] = np.sum(t * t, axis=2)
    return out


def pq_code_slack(residual, codebooks, codes, chunk=2048):
    """For every (row, subspace): (float64 distance of the STORED code) - (minimum over the 256 codewords), and the derived f32
    bound on that difference.  pq_assign_kernel computes r = x - c (one rounding: |dr| <= u |r|), t = r - a (|dt| <= u|r| + u|t|),
    d = sum of 8 squares: |d^ - d| <= gamma_12 sum t^2 + 3u sum |t||r|  (2 t dt + the square's rounding + 8 additions)."""
    r = np.asarray(residual, dtype=np.float64).reshape(-1, PQ_M, PQ_DSUB)
    cb = np.asarray(codebooks, dtype=np.float64)
    n = r.shape[0]
    slack, bound = np.empty((n, PQ_M)), np.empty((n, PQ_M))
    sub = np.arange(PQ_M)[None, :]

    def one(rr, code):
        t = rr - cb[sub, code]                                                   # [n][32][8]
        return np.sum(t * t, axis=2), gamma(12) * np.sum(t * t, axis=2) + 3 * U32 * np.sum(np.abs(t) * np.abs(rr), axis=2)

    for b in range(0, n, chunk):
        rr = r[b:b + chunk]
        best = np.argmin(pq_nearest(rr, cb), axis=2)
        d_st, b_st = one(rr, codes[b:b + chunk].astype(np.int64))
        d_mn, b_mn = one(rr, best)
        slack[b:b + chunk], bound[b:b + chunk] = d_st - d_mn, b_st + b_mn
    return slack, bound


def lpca_codes(x_rows, list_ids, ix):
    """Kind 1, the documented quantiser (lpca_encode_kernel): code_k = clamp(rint(Q_l[k] . (x - c_l) / scale_l[k]), -127, 127),
    rint = round half to even, in float64.  Returns int64 [n][32] (the file stores them as two's-complement bytes)."""
    c = ix["centroids"].astype(np.float64)[list_ids]
    r = np.asarray(x_rows, dtype=np.float64) - c
    out = np.empty((len(r), LP_DIMS), dtype=np.int64)
    basis, lscale = ix["basis"], ix["lscale"]
    for l in np.unique(list_ids):
        m = list_ids == l
        y = r[m] @ basis[l].astype(np.float64).T
        out[m] = np.clip(np.rint(y / lscale[l].astype(np.float64)[None, :]), -127, 127).astype(np.int64)
    return out


def unit64(q):
    q = np.asarray(q, dtype=np.float64)
    n = np.linalg.norm(q)
    return q / n if n > 0 else q


def adc_distance(q, ix, list_id):
    """float64 ADC distance max(1 - score, 0) of every row of list `list_id` to the query (brought to unit length, as the search
    does), in list order, from the file's own arrays:
      kind 0: score = q^.c_l + sum_s <q^_s, codebook[s][code_s]>                         (ivfpq.h; ivf_lut_kernel)
      kind 1: score = q^.c_l + sum_k scale_l[k] (Q_l[k] . q^) code_k, code_k signed      (lpca_project_kernel)
    Returns (distance, bound): bound is the derived f32 error of the kernel's value of that distance (see adc_bound_* below)."""
    qh = unit64(q)
    b, e = int(ix["offsets"][list_id]), int(ix["offsets"][list_id + 1])
    codes = ix["codes"][b:e]
    c = ix["centroids"][list_id].astype(np.float64)
    base = float(qh @ c)
    cnh = 0.5 * float(c @ c)
    # base = cnorm_half - (cnorm_half - q^.c) as the probe leaves it: the dot's bound, the unit query's, two subtractions
    base_err = (F32_COEF + UNIT_QUERY_COEF) * float(np.abs(qh) @ np.abs(c)) + 4 * U32 * (abs(base) + 2 * cnh)
    if ix["kind"] == 0:
        lut = np.einsum("sd,skd->sk", qh.reshape(PQ_M, PQ_DSUB), ix["codebooks"].astype(np.float64))          # [32][256]
        lut_abs = np.einsum("sd,skd->sk", np.abs(qh).reshape(PQ_M, PQ_DSUB), np.abs(ix["codebooks"].astype(np.float64)))
        terms = lut[np.arange(PQ_M)[None, :], codes]                                                            # [n][32]
        score = base + terms.sum(axis=1)
        # each LUT entry: an 8-term f32 dot of the f32 unit query; then 33 values added one after the other
        err = base_err + (gamma(PQ_DSUB) + UNIT_QUERY_COEF) * lut_abs[np.arange(PQ_M)[None, :], codes].sum(axis=1) \
            + gamma(PQ_M + 1) * (abs(base) + np.abs(terms).sum(axis=1))
    else:
        Q = ix["basis"][list_id].astype(np.float64)
        sc = ix["lscale"][list_id].astype(np.float64)
        w = sc * (Q @ qh)
        w_err = np.abs(sc) * (F32_COEF + UNIT_QUERY_COEF) * (np.abs(Q) @ np.abs(qh)) + U32 * np.abs(w)
        signed = codes.view(np.int8).astype(np.float64)
        score = base + signed @ w
        # the kernel adds w_k * (code_k + 128) and takes 128 * sum(w) off the base: 32 + 32 + 2 additions of values bounded by
        # |base| + 256 sum |w|, on weights that carry w_err each
        err = base_err + 256.0 * w_err.sum() + gamma(2 * PQ_M + 4) * (abs(base) + 256.0 * np.abs(w).sum()) + np.zeros(len(codes))
    # d = max(1 - score * (1/|q^|), 0): the f32 unit query's length is 1 within gamma_260, two more roundings
    err = err + (UNIT_QUERY_COEF + 4 * U32) * (1.0 + np.abs(score))
    return np.maximum(1.0 - score, 0.0), err


def probe_reference(q, centroids, nprobe):
    """The nprobe lists with the smallest 0.5|c|^2 - q^.c in float64 (ties -> smaller list id, as ivf_probe_select_kernel documents),
    and whether the choice is DECIDED: the nprobe-th and (nprobe+1)-th scores lie further apart than the two scores' f32 bounds
    (ivf_score_kernel: plain f32 products on the MFMA pipe, so dot_bound's gamma_256 with u = 2^-24, plus the unit query's rounding
    and the 0.5|c|^2 term)."""
    qh = unit64(q)
    c = np.asarray(centroids, dtype=np.float64)
    dot = c @ qh
    cnh = 0.5 * np.sum(c * c, axis=1)
    score = cnh - dot
    order = np.lexsort((np.arange(len(c)), score))
    if nprobe >= len(c):
        return np.sort(order), True
    err = score_bound(np.abs(c) @ np.abs(qh), dot, cnh, F32_COEF + UNIT_QUERY_COEF)
    a, b = order[nprobe - 1], order[nprobe]
    return np.sort(order[:nprobe]), bool(score[b] - score[a] > err[a] + err[b])


# ---------------------------------------------------------------------------------------------- corpora and a NumPy build
# the corpus of the GPU tests (test_gpu_ivf_structure.py, test_gpu_ivf_search_contract.py); test_ivf_ref_cpu.py checks what they need of it
GPU_N, GPU_NLIST, GPU_SEED, GPU_QSEED = 12288, 64, 41, 141


def iso_rows(n, seed):
    """n isotropic unit rows: no structure, so k-means cuts them into lists of similar size."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, DIM), dtype=np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True).astype(np.float32)
    return np.ascontiguousarray(x, dtype=np.float32)


def build_sample(n, nlist, train_sample=0):
    """(rows of the training sample, rows of the starting centroids) as smt_ivfpq_build documents them: S = train_sample or
    64 nlist, clamped to [nlist, N]; sample row i = corpus row i * (N / S); starting centroid l = sample row l * (S / nlist)."""
    S = train_sample if train_sample else 64 * nlist
    S = max(min(S, n), nlist)
    stride = n // S
    return np.arange(S) * stride, np.arange(nlist) * stride * (S // nlist)


def numpy_kmeans(x, nlist, iters, train_sample=0):
    """Lloyd iterations in float64 on the build's sample from the build's starting rows (an empty list keeps its centroid)."""
    x = np.asarray(x, dtype=np.float64)
    sample, start = build_sample(len(x), nlist, train_sample)
    c = x[start].copy()
    xs = x[sample]
    for _ in range(iters):
        a = np.argmax(assign_scores(xs, c), axis=1)
        for l in range(nlist):
            m = a == l
            if m.any():
                c[l] = xs[m].mean(axis=0)
    return c


def contenders(x, centroids, coef):
    """Boolean [n][nlist]: centroid c may be the one a kernel with score bound `coef` assigns the row to -- its float64 score is
    within the two bounds of the best one.  A row with one contender is decided; more than one is a near-tie."""
    x64, c64 = np.asarray(x, dtype=np.float64), np.asarray(centroids, dtype=np.float64)
    dot = x64 @ c64.T
    cnh = 0.5 * np.sum(c64 * c64, axis=1)[None, :]
    score = dot - cnh
    err = score_bound(pair_abs(x64, c64), dot, cnh, coef)
    best = np.argmax(score, axis=1)
    rows = np.arange(len(x64))
    return score >= (score[rows, best] - err[rows, best])[:, None] - err
