"""Cases and references of the pooled-lookup sweep (tests/test_pool_sweep_ref.py
on the CPU, tests/test_gpu_pool_sweep.py on the GPU).  numpy only.

Every pooled entry of csrc/pool.hip and csrc/grad_rows.hip picks a kernel
instantiation <VEC, G, CPL> from the row width: a row is covered by a group of
G lanes, lane lg owning the CPL chunks lg + c * G of VEC floats each
(dr_rows.h).  Inside pool_bag the path also depends on the bag length.  This
module restates those choices in Python (the class maps and the path
predicates), derives from them the widths and bag lengths a sweep has to
visit, builds the cases, and states three references of the pooled operation:

 (a) the CPU oracle (oracle/), passed in by the tests;
 (b) a float64 restatement with a rounding-count error bound (below);
 (c) integer-valued tables, whose fp32 sums are exact in any order.

Error bounds.  u = 2^-24 is the unit roundoff of fp32 (half an ulp, relative).
A value that passes through c roundings carries a relative error of at most
c * u to first order, so a sum of terms t_k, each of which passes through at
most c roundings on its way into the result, is within c * u * sum |t_k| of
the exact sum.  Every bound here is (c + 1) * u * sum |t_k|: the count c is
stated next to the code that uses it, and the one extra unit covers the
rounding of the divisor sqrt(n) and the second-order terms (c * u <= 1e-4
at the sizes of the sweep, so they are far below one unit).
"""
import functools

import numpy as np

U = 2.0 ** -24
COMBINERS = ("sum", "mean", "sqrtn")
TABLE_ROWS = 300          # rows of every table of the sweep
MAX_DIM = 1100            # the ladders are scanned over 1 .. MAX_DIM


# ---------------------------------------------------------------------------
# Class maps: (VEC, G, CPL) per width, None = the entry refuses the width
# ---------------------------------------------------------------------------
def _ladder(x, steps):
    for limit, cls in steps:
        if x <= limit:
            return cls
    return None


def pool_class(dim):
    """dispatch_pool<ORDER> (pool.hip): the fp32 pooled forward, both orders."""
    if dim % 4 == 0:
        return _ladder(dim // 4, [(1, (4, 1, 1)), (2, (4, 2, 1)), (4, (4, 4, 1)), (8, (4, 8, 1)),
                                  (16, (4, 16, 1)), (32, (4, 32, 1)), (64, (4, 64, 1)),
                                  (128, (4, 64, 2)), (256, (4, 64, 4))])
    return _ladder(dim, [(4, (1, 4, 1)), (8, (1, 8, 1)), (16, (1, 16, 1)), (32, (1, 32, 1)),
                         (64, (1, 64, 1)), (256, (1, 64, 4))])


def pool_class_bf16(dim):
    """dispatch_pool_bf16 (pool.hip) behind dr_pool_grouped_ex's dim % 8 == 0:
    the class of the general kernel, VEC = 4 bf16 values per chunk."""
    if dim % 8:
        return None
    return _ladder(dim // 4, [(4, (4, 4, 1)), (8, (4, 8, 1)), (16, (4, 16, 1)), (32, (4, 32, 1)),
                              (64, (4, 64, 1)), (128, (4, 64, 2)), (256, (4, 64, 4))])


def csr_class(dim):
    """dispatch_csr_sum (pool.hip) with src_stride == dim: SparseSegment*Grad
    and UnsortedSegmentSum."""
    if dim % 4 == 0:
        return _ladder(dim // 4, [(2, (4, 2, 1)), (4, (4, 4, 1)), (8, (4, 8, 1)), (16, (4, 16, 1)),
                                  (32, (4, 32, 1)), (64, (4, 64, 1)), (256, (4, 64, 4))])
    return _ladder(dim, [(8, (1, 8, 1)), (32, (1, 32, 1)), (64, (1, 64, 1)), (256, (1, 64, 4))])


def grad_class(dim):
    """dr_pool_grad_grouped (pool.hip): the Unique-path backward, 16-byte
    aligned gradients with top_stride % 4 == 0 when dim % 4 == 0."""
    if dim > 1024:      # kGradMaxDim
        return None
    if dim % 4 == 0:
        return _ladder(dim // 4, [(8, (4, 8, 1)), (16, (4, 16, 1)), (32, (4, 32, 1)),
                                  (64, (4, 64, 1)), (256, (4, 64, 4))])
    return _ladder(dim, [(64, (1, 64, 1)), (256, (1, 64, 4))])


def rows_class(dim):
    """The launch_rows dispatch of dr_pool_grad_rows_grouped_ex2
    (grad_rows.hip): the row-grouped backward."""
    if dim > 1024:      # kRowsMaxDim
        return None
    if dim % 4 == 0:
        return _ladder(dim // 4, [(8, (4, 8, 1)), (16, (4, 16, 1)), (32, (4, 32, 1)),
                                  (64, (4, 64, 1)), (256, (4, 64, 4))])
    return _ladder(dim, [(4, (1, 4, 1)), (32, (1, 32, 1)), (64, (1, 64, 1)), (256, (1, 64, 4)),
                         (1024, (1, 64, 16))])


def gather_class(dim, aligned=True):
    """gather_dispatch<false> behind dr_gather (pool.hip); aligned: table and
    output 16-byte aligned."""
    if dim > 1024:
        return None
    if dim % 4 == 0 and aligned:
        return _ladder(dim // 4, [(4, (4, 4, 1)), (8, (4, 8, 1)), (16, (4, 16, 1)),
                                  (32, (4, 32, 1)), (64, (4, 64, 1)), (256, (4, 64, 4))])
    return _ladder(dim, [(8, (1, 8, 1)), (32, (1, 32, 1)), (64, (1, 64, 1)), (256, (1, 64, 4))])


def clip_grad_class(dim):
    """The DR_CLIPG ladder of dr_clip_by_norm_grad (pool.hip), aligned
    pointers when dim % 4 == 0."""
    if dim > 1024:
        return None
    if dim % 4 == 0:
        return _ladder(dim // 4, [(8, (4, 8, 1)), (16, (4, 16, 1)), (32, (4, 32, 1)),
                                  (64, (4, 64, 1)), (256, (4, 64, 4))])
    return _ladder(dim, [(64, (1, 64, 1)), (256, (1, 64, 4)), (1024, (1, 64, 16))])


LADDERS = {"pool": pool_class, "pool_bf16": pool_class_bf16, "csr": csr_class,
           "grad": grad_class, "rows": rows_class, "gather": gather_class,
           "clip_grad": clip_grad_class}


def _accepts(cls_fn, dim):
    if cls_fn is pool_class_bf16 and dim % 8:
        return None       # not a width of this ladder at all (a flag check, not the ladder)
    return cls_fn(dim)


def ladder_classes(cls_fn):
    """{(aligned, class): [widths]} over 1 .. MAX_DIM; aligned = dim % 4 == 0
    (the two halves of a ladder share class triples only by name)."""
    out = {}
    for dim in range(1, MAX_DIM + 1):
        c = _accepts(cls_fn, dim)
        if c is not None:
            out.setdefault((dim % 4 == 0, c), []).append(dim)
    return out


def lane0_widths(cls, lo, hi):
    """Widths of a CPL > 1 class whose last used column chunk holds one
    vector, lane 0's: dim = VEC * (k * G + 1), k = 1 .. CPL - 1 (260 -> dv = 65)."""
    vec, g, cpl = cls
    return [vec * (k * g + 1) for k in range(1, cpl) if lo <= vec * (k * g + 1) <= hi]


def class_widths(cls_fn):
    """The sweep of one ladder: the smallest and the largest width of every
    class, and for CPL > 1 the lane-0-only widths."""
    ws = set()
    for (_, cls), dims in ladder_classes(cls_fn).items():
        ws.update((dims[0], dims[-1]))
        if cls[2] > 1:
            usable = [w for w in lane0_widths(cls, dims[0], dims[-1]) if w in dims]
            ws.update(usable)
    return sorted(ws)


def first_refused(cls_fn, aligned):
    """The first width past the ladder's last class (aligned: dim % 4 == 0);
    None when the ladder refuses nothing up to MAX_DIM."""
    last = max(dims[-1] for (al, _), dims in ladder_classes(cls_fn).items() if al == aligned)
    for dim in range(last + 1, MAX_DIM + 1):
        if (dim % 4 == 0) != aligned:
            continue
        if cls_fn is pool_class_bf16 and dim % 8:
            continue
        return dim if cls_fn(dim) is None else None
    return None


POOL_WIDTHS = class_widths(pool_class)
BF16_WIDTHS = class_widths(pool_class_bf16)
CSR_WIDTHS = class_widths(csr_class)
GRAD_WIDTHS = class_widths(grad_class)
ROWS_WIDTHS = class_widths(rows_class)
CLIP_GRAD_WIDTHS = class_widths(clip_grad_class)
# dr_gather (width, 16-byte aligned table): both ends of its range, an unaligned
# table wherever the entry takes one
GATHER_CASES = [(1, False), (3, False), (4, True), (4, False), (255, False), (256, True),
                (256, False), (260, True), (1024, True)]
# max_norm: the norm is summed over the G lanes (group_sum<G>), right only if
# the idle lanes of a ragged width hold zeros
MAXNORM_WIDTHS = [20, 36, 68, 132, 260, 516, 5, 17, 65]


# ---------------------------------------------------------------------------
# Bag lengths and the path predicates of pool_bag / ali_bag_rows
# ---------------------------------------------------------------------------
def bag_lengths(G):
    """Bag lengths of a class of group width G: the ALI branches, every
    num % 8 residue, and for G >= 8 the BagPtrs window edges with 4G + 1, the
    first bag on the select_row path."""
    lens = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 16, 17}
    if G >= 8:
        lens |= {G, G + 1, 2 * G + 1, 3 * G + 1, 4 * G, 4 * G + 1}
    return sorted(lens)


def bag_path(G, num):
    """pool_bag (pool.hip), unweighted: 'empty', 'win<w>' = the highest
    BagPtrs window read (windows below it are read too), or 'select_row'."""
    if num <= 0:
        return "empty"
    if G >= 8 and num <= 4 * G:
        return "win%d" % ((num - 1) // G)
    return "select_row"


def ali_branches(num, combiner):
    """ali_bag_rows (dr_pool_order.h): the set of branches a bag takes."""
    if num <= 0:
        return {"empty"}
    if num == 1:
        return {"copy"}
    r = num % 8
    out = {"res%d" % r}
    first = 8 if r == 0 else (9 if r == 1 else r)
    if num > first:
        out.add("chunks_of_8")
    if combiner != "sum":
        out.add("div_first" if num < 10 else "div_total")
    return out


# ---------------------------------------------------------------------------
# Cases
# ---------------------------------------------------------------------------
class Case(object):
    """One launch: `lens` ids per bag over a table of TABLE_ROWS rows.

    Bags 0..7 hold one id each: a full chunk (kChunkNB = 8) that
    pool_fast_kernel takes and the general kernel must skip.  The bag-length
    list follows, and the batch is not a multiple of 8, so the ragged last
    chunk goes to the general kernel."""

    def __init__(self, dim, G, seed, kind, empty=True):
        rng = np.random.default_rng([seed, dim, G])
        lens = [1] * 8 + [n for n in bag_lengths(G) if n or empty]
        if len(lens) % 8 == 0:
            lens.append(3)
        self.dim, self.G, self.kind = dim, G, kind
        self.lens = np.asarray(lens, np.int64)
        self.B = len(lens)
        self.off = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int32)
        self.n = int(self.off[-1])
        self.seg = np.repeat(np.arange(self.B), self.lens).astype(np.int32)
        self.pos = np.concatenate([np.arange(l) for l in lens]).astype(np.int64)
        self.ind = np.stack([self.seg.astype(np.int64), self.pos], 1)
        self.ids = rng.integers(0, TABLE_ROWS, self.n).astype(np.int64)
        if kind == "int":
            # |sum| <= 257 * 64 * 3 < 2^24: every fp32 partial sum is an integer
            # below 2^24, exact in any association order
            self.table = rng.integers(-64, 65, (TABLE_ROWS, dim)).astype(np.float32)
            self.weights = rng.integers(1, 4, self.n).astype(np.float32)
        else:
            t = rng.standard_normal((TABLE_ROWS, dim))
            if kind == "clip":
                # positive entries (a relative tolerance against the oracle means
                # something without cancellation) and row norms spread by a
                # factor of 4, so that max_norm clips about half of the rows
                t = (np.abs(t) + 0.25) * np.linspace(0.5, 2.0, TABLE_ROWS)[:, None]
            self.table = t.astype(np.float32)
            self.weights = rng.uniform(0.25, 2.0, self.n).astype(np.float32)
        self.grad = rng.standard_normal((self.B, dim)).astype(np.float32)
        self.max_norm = None
        if kind == "clip":
            self.max_norm, self.norm_gap = pick_max_norm(self.table)


def pick_max_norm(table):
    """A max_norm in the widest gap between the sorted row norms of the
    table's middle half: about half of the rows are clipped, and no norm is
    near the threshold, where the clip's gradient jumps.  Returns (max_norm,
    relative distance to the nearest norm)."""
    nrm = np.sort(np.sqrt((table.astype(np.float64) ** 2).sum(1)))
    q = len(nrm) // 4
    mid = nrm[q:len(nrm) - q]
    k = int(np.argmax(np.diff(mid)))
    c = float(np.float32(0.5 * (mid[k] + mid[k + 1])))
    return c, float(np.abs(nrm - c).min() / c)


@functools.lru_cache(maxsize=None)
def make_case(dim, G, kind="rand", empty=True, seed=20240611):
    return Case(dim, G, seed, kind, empty)


class BackCase(object):
    """One backward: 37 bags of 0 .. 17 ids over a small vocabulary, so that an
    id's run (the positions that share it) is 1, 2, a handful or a few dozen
    positions long; the long-run walkers have their own tests."""

    def __init__(self, dim, seed):
        rng = np.random.default_rng([seed, dim])
        lens = [0, 1, 2, 3, 9, 10, 17, 8, 1, 1] + rng.integers(1, 7, 27).tolist()
        self.dim = dim
        self.lens = np.asarray(lens, np.int64)
        self.B = len(lens)
        self.off = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int32)
        self.n = int(self.off[-1])
        self.seg = np.repeat(np.arange(self.B), self.lens).astype(np.int32)
        pos = np.concatenate([np.arange(l) for l in lens]).astype(np.int64)
        self.ind = np.stack([self.seg.astype(np.int64), pos], 1)
        ids = rng.integers(3, 150, self.n)
        hot = rng.random(self.n)
        ids[hot < 0.45] = rng.integers(1, 3, int((hot < 0.45).sum()))   # two ids, ~25 each
        ids[hot < 0.25] = 0                                             # one id, ~30 positions
        self.ids = ids.astype(np.int64)
        # unique ids in first-occurrence order, idx = position -> unique row
        _, first, inv = np.unique(self.ids, return_index=True, return_inverse=True)
        rank = np.empty(len(first), np.int64)
        rank[np.argsort(first)] = np.arange(len(first))
        self.idx = rank[inv].astype(np.int32)
        self.uids = self.ids[np.sort(first)]
        self.U = len(first)
        self.runs = np.bincount(self.idx)
        self.grad = rng.standard_normal((self.B, dim)).astype(np.float32)
        self.weights = rng.uniform(0.25, 2.0, self.n).astype(np.float32)
        self.int_grad = rng.integers(-64, 65, (self.B, dim)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def backward_case(dim, seed=20240612):
    return BackCase(dim, seed)


def forward_case(dim, kind="rand"):
    return make_case(dim, pool_class(dim)[1], kind)


def seq_case(dim, kind="rand"):
    """The fused op (ORDER_SEQ) follows fill_empty_rows in the reference: its
    restatement gives an empty bag no meaning, so these cases hold none."""
    return make_case(dim, pool_class(dim)[1], kind, empty=False)


def bf16_case(dim, kind="rand"):
    return make_case(dim, pool_class_bf16(dim)[1], kind)


# ---------------------------------------------------------------------------
# (b) float64 restatements with their bounds, (c) exact integer sums
# ---------------------------------------------------------------------------
def clip64(rows, max_norm):
    """clip_by_norm of every row in float64: x * c / max(|x|, c) -- the ALI
    order's formula; the fused op's `l2 > c ? x * (c / l2) : x` is the same
    function."""
    l2 = np.sqrt((rows * rows).sum(1, keepdims=True))
    return rows * max_norm / np.maximum(l2, max_norm)


def clip_roundings(dim):
    """Roundings on the way of one element through the clip: the squared
    norm is dim products and dim - 1 adds of positive terms (relative error
    dim * u whatever the order), halved by the square root -> dim / 2; then
    the square root, row * max_norm and the division: 3."""
    return dim / 2.0 + 3.0


def forward_ref(table, ids, off, combiner, weights=None, max_norm=None):
    """Pooled bags in float64 -> (ref [B, D], bound [B, D]).

    Rounding count of one term on its way into the result, n = bag length:
     * unweighted: n - 1 adds and one divide = n, so (n + 1) * u;
     * weighted sum: one multiply and n - 1 adds = n;
     * weighted mean: those n, the divide, and the weight sum's n - 1 adds
       (weights are positive: the sum's relative error is (n - 1) * u) = 2n;
     * weighted sqrtn: those n, the divide, and sqrt(sum w^2): one multiply
       and n - 1 adds per weight, halved by the square root, plus the square
       root itself = n + 1 + n / 2 + 1;
     * max_norm: clip_roundings(dim) more.
    An empty bag is exactly zero, or NaN under weights with mean / sqrtn."""
    table = np.asarray(table, np.float64)
    B, D = len(off) - 1, table.shape[1]
    rows = table[ids]
    extra = 0.0
    if max_norm is not None:
        rows = clip64(rows, float(max_norm))
        extra = clip_roundings(D)
    ref = np.zeros((B, D))
    bound = np.zeros((B, D))
    for b in range(B):
        k0, k1 = int(off[b]), int(off[b + 1])
        n = k1 - k0
        if n == 0:
            if weights is not None and combiner != "sum":
                ref[b] = np.nan
                bound[b] = np.nan
            continue
        x = rows[k0:k1]
        if weights is None:
            q = {"sum": 1.0, "mean": float(n), "sqrtn": np.sqrt(n)}[combiner]
            count = n
        else:
            w = np.asarray(weights[k0:k1], np.float64)
            x = x * w[:, None]
            q = {"sum": 1.0, "mean": w.sum(), "sqrtn": np.sqrt((w * w).sum())}[combiner]
            count = {"sum": n, "mean": 2 * n, "sqrtn": 1.5 * n + 2}[combiner]
        ref[b] = x.sum(0) / q
        bound[b] = (count + extra + 1) * U * np.abs(x).sum(0) / q
    return ref, bound


def int_sum_ref(table, ids, off, weights=None):
    """(c): the int64 sum of every bag of an integer-valued table."""
    t = np.asarray(table).astype(np.int64)
    rows = t[ids]
    if weights is not None:
        rows = rows * np.asarray(weights).astype(np.int64)[:, None]
    out = np.zeros((len(off) - 1, t.shape[1]), np.int64)
    for b in range(len(off) - 1):
        out[b] = rows[off[b]:off[b + 1]].sum(0)
    return out


def _scatter(idx, terms, U_rows):
    out = np.zeros((U_rows, terms.shape[1]))
    np.add.at(out, idx, terms)
    return out


def segment_grad_ref(grad, idx, seg, lens, U_rows, combiner):
    """SparseSegment{Sum,Mean,SqrtN}Grad in float64 -> (ref, bound), out[u] =
    sum over the positions k with idx[k] == u of grad[seg[k]] * scale, scale =
    1, 1 / n or 1 / sqrt(n) of position k's bag.  Count of a run of m
    positions: m - 1 adds; mean / sqrtn add the rounding of the scale and the
    multiply by it = m + 1."""
    n = np.asarray(lens, np.float64)[seg]
    scale = {"sum": np.ones_like(n), "mean": 1.0 / n, "sqrtn": 1.0 / np.sqrt(n)}[combiner]
    terms = np.asarray(grad, np.float64)[seg] * scale[:, None]
    m = np.bincount(idx, minlength=U_rows).astype(np.float64)[:, None]
    count = np.maximum(m - 1, 0) + (0 if combiner == "sum" else 2)
    return _scatter(idx, terms, U_rows), (count + 1) * U * _scatter(idx, np.abs(terms), U_rows)


def weighted_grad_ref(grad, idx, seg, weights, off, U_rows, combiner):
    """Backward of the weighted composition (embedding_ops.py:609-651) in
    float64 -> (ref, bound): out[u] = sum_k grad[seg[k]] / den(bag) * w[k], den
    = 1, sum w or sqrt(sum w^2).  Count of term k in a run of m: the m - 1
    adds, the multiply by w, and for mean / sqrtn the divide and the
    divisor's own error, n - 1 (mean) or n / 2 + 2 (sqrtn: a product and n - 1
    adds per weight, halved, the square root) for a bag of n."""
    w = np.asarray(weights, np.float64)
    B = len(off) - 1
    n = np.diff(off).astype(np.float64)
    if combiner == "sum":
        den, c_bag = np.ones(B), np.zeros(B)
    elif combiner == "mean":
        den, c_bag = _scatter(seg, w[:, None], B)[:, 0], n - 1 + 1
    else:
        den, c_bag = np.sqrt(_scatter(seg, (w * w)[:, None], B)[:, 0]), n / 2 + 2 + 1
    den = np.where(n > 0, den, 1.0)
    terms = np.asarray(grad, np.float64)[seg] / den[seg][:, None] * w[:, None]
    m = np.bincount(idx, minlength=U_rows).astype(np.float64)[:, None]
    per_term = (c_bag[seg] + 1)[:, None] * np.abs(terms)
    bound = U * (_scatter(idx, per_term, U_rows) + (np.maximum(m - 1, 0) + 1) *
                 _scatter(idx, np.abs(terms), U_rows))
    return _scatter(idx, terms, U_rows), bound


def unsorted_segment_sum_ref(data, seg, num_segments):
    """UnsortedSegmentSum in float64 (negative ids are skipped) -> (ref,
    bound); count of a segment of m rows: m - 1 adds."""
    keep = seg >= 0
    d = np.asarray(data, np.float64)[keep]
    s = seg[keep]
    m = np.bincount(s, minlength=num_segments).astype(np.float64)[:, None]
    return (_scatter(s, d, num_segments),
            (np.maximum(m - 1, 0) + 1) * U * _scatter(s, np.abs(d), num_segments))


def clip_by_norm_grad_ref(rows, grad, max_norm):
    """Gradient of clip_by_norm (clip_ops.py:164-184) in float64 -> (ref,
    bound).  With m = max(|x|, c): out = g * c / m + 2 * gs * x, gs = gl2 / (2
    |x|), gl2 = -sum_d g_d x_d c / m^2 where |x| >= c, else 0.

    Counts (D = dim).  m carries D / 2 + 1 (the norm, as in clip_roundings).
    a = g / m * c: two roundings and m's -> D / 2 + 3.  A term of gl2 is four
    roundings (x * c, / m, / m, * g), m's error twice and D - 1 adds -> 2 D +
    5; gs adds the divide by |x| and its error, b = gs * x one multiply -> 2.5
    D + 8.  out = (a + b) + b: two more adds on every part.  The terms of gl2
    may cancel, so its bound is on the sum of their magnitudes."""
    x = np.asarray(rows, np.float64)
    g = np.asarray(grad, np.float64)
    c = float(max_norm)
    D = x.shape[1]
    l2 = np.sqrt((x * x).sum(1, keepdims=True))
    m = np.maximum(l2, c)
    a = g * c / m
    clipped = l2 >= c
    safe = np.where(l2 > 0, l2, 1.0)
    gl2 = np.where(clipped, -(g * x).sum(1, keepdims=True) * c / (m * m), 0.0)
    gl2_abs = np.where(clipped, np.abs(g * x).sum(1, keepdims=True) * c / (m * m), 0.0)
    b = 0.5 * gl2 / safe * x
    b_abs = 0.5 * gl2_abs / safe * np.abs(x)
    bound = U * ((D / 2 + 3 + 2 + 1) * np.abs(a) + (2.5 * D + 8 + 2 + 1) * 2 * b_abs)
    return a + 2 * b, bound


def within(got, ref, bound):
    """|got - ref| <= bound elementwise, NaN matching NaN; returns the worst
    ratio |got - ref| / bound (0 where both are exact)."""
    got = np.asarray(got, np.float64)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), "NaN pattern differs"
    err = np.abs(np.where(nan, 0.0, got - ref))
    bnd = np.where(nan, 0.0, bound)
    bad = err > bnd
    assert not bad.any(), "outside the float64 bound at %s: err %g bound %g" % (
        np.argwhere(bad)[0].tolist(), err[bad][0], bnd[bad][0])
    pos = bnd > 0
    return float((err[pos] / bnd[pos]).max()) if pos.any() else 0.0
