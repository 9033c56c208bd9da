"""A CPU model of mobgs_amd/csrc/wave_shared.h and reduce_shared.h, restated from the headers' comments and statements:
which lanes meet at each step, the association order of the additions in the primitive's own precision, and where the
results lie afterwards.  numpy only; nothing of the package is imported, so the model cannot inherit a mistake from it.

Shapes.  The lane (thread) axis is the LAST axis inside the model functions.  A case's input table is (G, T, KI) and its
expected output (G, T, KO), as mobgs_lane_probe lays them out: G groups, T threads per group, KI / KO values per thread.

The tables the CPU and GPU tests share live here too: counting vectors (exact in any order: they show that each lane is
counted once and where the total lands), placement vectors (each output register names its component), order-sensitive
vectors (about 30 binades, mixed signs, seeded; drawn until the documented order, the left-to-right sum and the other
pairing tree all give different bits) and specials (signed zeros, infinities, a NaN, INT_MIN / INT_MAX, denormals)."""
import functools

import numpy as np

WAVE = 64
BLOCK = 256                 # the one workgroup size block_sum / rows_sum are instantiated with
WAVES = BLOCK // WAVE
LANES = np.arange(WAVE)
BUTTERFLY_BITS = (5, 4, 3, 2, 1, 0)     # MOBGS_WAVE_FOLD: xor 32 down to xor 1
ROW_FIRST_BITS = (0, 1, 2, 3, 4, 5)
ROW_BITS = (0, 1, 2, 3)                 # row_allreduce: xor 1, xor 2, half mirror (the other quad pair), ror 8
HALF_BITS = (0, 1, 2, 3, 4)             # half_wave_sum: the row, then xor 16
ALLREDUCE_BITS = (5, 4, 0, 1, 2, 3)     # wave_allreduce, wave_reduce_components: swap 32, swap 16, then the row
PAIR_BITS = (5, 0, 1, 2, 3, 4)          # wave_reduce_pair: swap 32, the row, swap 16
NVPS = (8, 16, 32, 64)
ROW_COUNTS = (0, 1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 3)
STRIDES = (1, 2)
N_ORDER = 16                # order-sensitive vectors per primitive


def _quiet(fn):
    @functools.wraps(fn)
    def wrapped(*a, **k):
        with np.errstate(all="ignore"):
            return fn(*a, **k)
    return wrapped


# ---- the lane a DPP control reads, for every lane of the wave -----------------------------------------------------------
DPP_SRC = {
    0xB1: LANES ^ 1,                                   # quad_perm:[1,0,3,2]
    0x4E: LANES ^ 2,                                   # quad_perm:[2,3,0,1]
    0x1B: (LANES & ~3) | (3 - (LANES & 3)),            # quad_perm:[3,2,1,0]
    0x141: (LANES & ~7) | (7 - (LANES & 7)),           # row_half_mirror
    0x128: (LANES & ~15) | ((LANES - 8) & 15),         # row_ror:8 = lane ^ 8
    0x124: (LANES & ~15) | ((LANES - 4) & 15),         # row_ror:4: lane l reads lane l - 4 of its row, cyclically
}


def dpp_mov(v, ctrl, src=DPP_SRC):
    return v[..., src[ctrl]]


@_quiet
def dpp_add(v, ctrl, src=DPP_SRC):
    return v + v[..., src[ctrl]]


@_quiet
def dpp_add_xor4(v):
    """v + (up + dn): banks {0, 2} take lane + 4 through row_shl:4, banks {1, 3} lane - 4 through row_shr:4, and the shift
    that is not the lane's own gives an exact +0 -- so a partner of -0 arrives as (-0) + (+0) = +0."""
    low = (LANES & 4) == 0
    zero = np.zeros((), v.dtype)
    up = np.where(low, v[..., (LANES + 4) & 63], zero)
    dn = np.where(~low, v[..., (LANES - 4) & 63], zero)
    return v + (up + dn)


# ---- xor butterflies -------------------------------------------------------------------------------------------------------
def add(a, b):
    return a + b


def fmin(a, b):
    """min of the device: fminf for floats (a NaN loses against a number, -0 < +0), the integer minimum otherwise."""
    if a.dtype.kind != "f":
        return np.minimum(a, b)
    a_wins = (a < b) | ((a == b) & np.signbit(a)) | np.isnan(b)
    return np.where(np.isnan(a), b, np.where(a_wins, a, b))


def fmax(a, b):
    if a.dtype.kind != "f":
        return np.maximum(a, b)
    a_wins = (a > b) | ((a == b) & ~np.signbit(a)) | np.isnan(b)
    return np.where(np.isnan(a), b, np.where(a_wins, a, b))


@_quiet
def wave_fold(v, op):
    """MOBGS_WAVE_FOLD: v = OP(v, v of lane ^ off), off = 32, 16, .. 1: every lane ends with the same bits."""
    for bit in BUTTERFLY_BITS:
        v = op(v, v[..., LANES ^ (1 << bit)])
    return v


def wave_sum(v):
    return wave_fold(v, add)


def wave_min(v):
    return wave_fold(v, fmin)


def wave_max(v):
    return wave_fold(v, fmax)


# ---- DPP and permlane-swap reductions ---------------------------------------------------------------------------------------
def row_allreduce(v, src=DPP_SRC):
    for ctrl in (0xB1, 0x4E, 0x141, 0x128):
        v = dpp_add(v, ctrl, src)
    return v


@_quiet
def half_wave_sum(v):
    v = row_allreduce(v)
    return v + v[..., LANES ^ 16]


@_quiet
def swap32_add(a, b):
    """permlane32_swap(a, b) + add: lanes 0-31 get a[l] + a[l + 32], lanes 32-63 get b[l - 32] + b[l]."""
    return np.where(LANES < 32, a + a[..., LANES ^ 32], b + b[..., LANES ^ 32])


@_quiet
def swap16_add(a, b):
    """permlane16_swap(a, b) + add: even rows get a[l] + a[l + 16], odd rows b[l - 16] + b[l]."""
    return np.where((LANES & 16) == 0, a + a[..., LANES ^ 16], b + b[..., LANES ^ 16])


def wave_allreduce(v):
    v = swap32_add(v, v)
    v = swap16_add(v, v)
    return row_allreduce(v)


def wave_reduce_components(v):
    """v: (.., NVP, 64) -> (.., NVP / 4, 64): register k of every lane of row r holds the wave total of component
    component_of(nvp, r, k)."""
    nvp = v.shape[-2]
    s1 = [swap32_add(v[..., i, :], v[..., i + nvp // 2, :]) for i in range(nvp // 2)]
    s2 = [swap16_add(s1[i], s1[i + nvp // 4]) for i in range(nvp // 4)]
    return np.stack([row_allreduce(x) for x in s2], axis=-2)


def component_of(nvp, row, k):
    return (row >> 1) * (nvp // 2) + (row & 1) * (nvp // 4) + k


def wave_reduce_pair(e0, e1):
    """Lanes 0-31 hold the wave total of e0, lanes 32-63 that of e1."""
    x = row_allreduce(swap32_add(e0, e1))
    return swap16_add(x, x)


def wave_fence(v):
    """Lane l writes slot l; fence; reads slot 63 - l and writes that to slot (l + 17) & 63; fence; reads slot l."""
    first = v[..., 63 - LANES]
    slots = np.empty_like(v)
    slots[..., (LANES + 17) & 63] = first
    return np.stack([first, slots], axis=-1)


# ---- the fixed-order sums of reduce_shared.h ---------------------------------------------------------------------------------
@_quiet
def shfl_down_lane0(v):
    """Lane 0 of `v += __shfl_down(v, off)`, off = 32 .. 1 (a lane whose partner is past the wave reads itself): lanes
    [0, off) take part at each step, so lane 0 ends with the butterfly's own tree."""
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[..., np.where(LANES + off < WAVE, LANES + off, LANES)]
    return v[..., 0]


@_quiet
def block_sum(v):
    """v: (.., BLOCK) float64 -> (..,): thread 0's total: ((w0 + w1) + w2) + w3 of the waves' lane-0 values."""
    w = shfl_down_lane0(v.reshape(v.shape[:-1] + (WAVES, WAVE)))
    total = w[..., 0]
    for k in range(1, WAVES):
        total = total + w[..., k]
    return total


@_quiet
def block_sum4(v):
    """v: (.., 256) float32 -> (..,): every thread's total: a butterfly per wave, then ((w0 + w1) + w2) + w3."""
    w = wave_sum(v.reshape(v.shape[:-1] + (4, WAVE)))[..., 0]
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


@_quiet
def run_sums(p, n, stride, threads, ceil=True):
    """Thread t adds rows [t per, min(t per + per, n)) of p[r stride] in ascending order onto 0.0, per = ceil(n / threads)."""
    per = -(-n // threads) if ceil else n // threads
    t = np.arange(threads)
    s = np.zeros(p.shape[:-1] + (threads,), np.float64)
    for k in range(per):
        r = t * per + k
        s = np.where(r < n, s + p[..., np.minimum(r, n - 1) * stride], s)
    return s


def rows_sum(p, n, stride, ceil=True):
    return block_sum(run_sums(p, n, stride, BLOCK, ceil))


def wave_rows_sum(p, n, stride):
    return wave_sum(run_sums(p, n, stride, WAVE))[..., 0]


# ---- other orders, for the condition of the order-sensitive inputs ---------------------------------------------------------
@_quiet
def left_to_right(v):
    acc = v[..., 0]
    for i in range(1, v.shape[-1]):
        acc = acc + v[..., i]
    return acc


@_quiet
def tree_sum(v, bits):
    """Element 0 of the pairing tree that meets lane ^ (1 << b) for b in `bits`, in that order."""
    idx = np.arange(v.shape[-1])
    for b in bits:
        v = v + v[..., idx ^ (1 << b)]
    return v[..., 0]


@_quiet
def waves_in_order(v, bits):
    """A block sum with another tree inside each wave: tree_sum per wave, then the waves left to right."""
    w = tree_sum(v.reshape(v.shape[:-1] + (-1, WAVE)), bits)
    return left_to_right(w)


def bits_of(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ---- comparison: what the GPU test asserts with ------------------------------------------------------------------------------
def mismatches(out, expected, threads=None):
    """Indices (g, t, j) where out differs from expected: NaN results are compared as NaN-ness, everything else as bits.
    threads: the threads whose value the contract specifies (None: all)."""
    assert out.shape == expected.shape and out.dtype == expected.dtype, (out.shape, expected.shape, out.dtype, expected.dtype)
    bad = bits_of(out) != bits_of(expected)
    if expected.dtype.kind == "f":
        bad = np.where(np.isnan(expected), ~np.isnan(out), bad)
    if threads is not None:
        keep = np.zeros(out.shape[1], bool)
        keep[list(threads)] = True
        bad = bad & keep[None, :, None]
    return [tuple(int(i) for i in ix) for ix in np.argwhere(bad)]


def not_uniform(out, span):
    """Groups of `span` consecutive threads (64: the wave, 32: a half, 16: a row) that do not hold one bit pattern
    (NaNs count as one pattern)."""
    b = bits_of(out)
    if out.dtype.kind == "f":
        b = np.where(np.isnan(out), 0, b)
    b = b.reshape(b.shape[0], b.shape[1] // span, span, b.shape[2])
    return [tuple(int(i) for i in ix) for ix in np.argwhere((b != b[:, :, :1]).any(axis=2))]


# ---- input tables --------------------------------------------------------------------------------------------------------------
def counting(dtype, width=WAVE):
    """One-hot lanes (1 in lane w of vector w), all ones, and the lane index: exact in any order."""
    eye = np.eye(width, dtype=dtype)
    return np.concatenate([eye, np.ones((1, width), dtype), np.arange(width, dtype=dtype)[None]])


def _draw(rng, shape, dtype):
    mant = rng.uniform(1.0, 2.0, shape)
    expo = rng.integers(-15, 15, shape)
    sign = rng.choice([-1.0, 1.0], shape)
    return (sign * mant * np.exp2(expo)).astype(dtype)


def order_vectors(count, width, dtype, seed, model, others):
    """`count` seeded vectors of `width` values over about 30 binades, mixed signs, for which model(v) differs in bits from
    every other(v): a draw that does not separate the orders is drawn again."""
    rng = np.random.default_rng(seed)
    kept = []
    for _ in range(64):
        cand = _draw(rng, (max(4 * count, 64), width), dtype)
        want = bits_of(model(cand))
        ok = np.ones(len(cand), bool)
        for other in others:
            ok &= bits_of(other(cand)) != want
        kept.extend(cand[ok])
        if len(kept) >= count:
            return np.stack(kept[:count])
    raise AssertionError("the generator does not separate the orders")


def specials(dtype, width=WAVE):
    """Signed zeros, infinities, a NaN in one lane, denormals; INT_MIN / INT_MAX for the integers."""
    if np.dtype(dtype).kind == "i":
        info = np.iinfo(dtype)
        rows = np.zeros((4, width), dtype)
        rows[0, 5], rows[0, 40] = info.min, info.max
        rows[1, :] = info.max
        rows[1, 63] = info.min
        rows[2, :] = info.min
        rows[3, :] = -np.arange(width)
        rows[3, 17] = info.max
        return rows
    tiny = np.finfo(dtype).smallest_subnormal
    rows = np.zeros((9, width), dtype)
    rows[0, :] = -0.0                                  # all -0
    rows[1, 5] = -0.0                                  # one -0 among +0
    rows[2, :] = -0.0
    rows[2, 37] = 0.0                                  # one +0 among -0
    rows[3, :] = np.arange(width) - 20.0
    rows[3, 9] = np.inf
    rows[4, :] = np.arange(width) - 20.0
    rows[4, 50] = -np.inf
    rows[5, 3], rows[5, 60] = np.inf, -np.inf          # a sum of both is NaN
    rows[6, :] = np.arange(width) - 20.0
    rows[6, 37] = np.nan
    rows[7, :] = tiny * (np.arange(width) + 1)         # denormals, exact in any order
    rows[8, :] = tiny * (np.arange(width) - 30.0)      # denormals of both signs around -0 / +0
    rows[8, 30] = -0.0
    return rows


def placement(nvp):
    """(G, 64, nvp): component i of lane l carries (i + 1) 2^k, k = (l >> s) & 3 for one s per vector (wave totals
    240 (i + 1), with the half-wave groups 96 (i + 1): exact, below 2^24, pairwise distinct), then one vector per lane w in which only lane w carries i + 1."""
    i = np.arange(nvp, dtype=np.float32) + 1
    groups = [np.exp2((LANES >> s) & 3).astype(np.float32)[:, None] * i[None, :] for s in (0, 2, 4)]
    groups.append(np.exp2(LANES >> 5).astype(np.float32)[:, None] * i[None, :])
    one_hot = np.eye(WAVE, dtype=np.float32)[:, :, None] * i[None, None, :]
    return np.concatenate([np.stack(groups), one_hot])


def _tree(bits):
    return lambda v: tree_sum(v, bits)


@functools.lru_cache(maxsize=None)
def order_table(name):
    """The order-sensitive vectors of one primitive, (N, width) or, for the component reductions, (G, 64, KI)."""
    f32, f64 = np.float32, np.float64
    if name in ("wave_sum_f32", "wave_sum_f64"):
        return order_vectors(N_ORDER, WAVE, f32 if name.endswith("32") else f64, 11, _tree(BUTTERFLY_BITS),
                             (left_to_right, _tree(ROW_FIRST_BITS)))
    if name == "row_allreduce":       # four separating rows per vector
        rows = order_vectors(4 * N_ORDER, 16, f32, 12, _tree(ROW_BITS), (left_to_right, _tree(ROW_BITS[::-1])))
        return rows.reshape(N_ORDER, WAVE)
    if name == "half_wave_sum":
        halves = order_vectors(2 * N_ORDER, 32, f32, 13, _tree(HALF_BITS), (left_to_right, _tree(HALF_BITS[::-1])))
        return halves.reshape(N_ORDER, WAVE)
    if name == "wave_allreduce":
        return order_vectors(N_ORDER, WAVE, f32, 14, _tree(ALLREDUCE_BITS), (left_to_right, _tree(BUTTERFLY_BITS)))
    if name == "wave_reduce_pair":
        v = order_vectors(2 * N_ORDER, WAVE, f32, 15, _tree(PAIR_BITS), (left_to_right, _tree(BUTTERFLY_BITS)))
        return v.reshape(N_ORDER, 2, WAVE).transpose(0, 2, 1)
    if name.startswith("wave_reduce_components_"):
        nvp = int(name.rsplit("_", 1)[1])
        v = order_vectors(nvp * N_ORDER, WAVE, f32, 16 + nvp, _tree(ALLREDUCE_BITS), (left_to_right, _tree(BUTTERFLY_BITS)))
        return v.reshape(N_ORDER, nvp, WAVE).transpose(0, 2, 1)
    if name == "block_sum":
        return order_vectors(2 * N_ORDER, BLOCK, f64, 17, block_sum,
                             (left_to_right, lambda v: waves_in_order(v, ROW_FIRST_BITS)))
    if name == "block_sum4":
        return order_vectors(2 * N_ORDER, BLOCK, f32, 18, block_sum4,
                             (left_to_right, lambda v: waves_in_order(v, ROW_FIRST_BITS)))
    n = ROW_COUNTS[-1]
    if name == "rows_sum":
        return order_vectors(2 * N_ORDER, n, f64, 19, lambda p: rows_sum(p, n, 1),
                             (left_to_right, lambda p: waves_in_order(run_sums(p, n, 1, BLOCK), ROW_FIRST_BITS)))
    if name == "wave_rows_sum":
        return order_vectors(N_ORDER, n, f64, 20, lambda p: wave_rows_sum(p, n, 1),
                             (left_to_right, lambda p: tree_sum(run_sums(p, n, 1, WAVE), ROW_FIRST_BITS)))
    raise KeyError(name)


def strided(values, n, stride):
    """(.., >= n) -> (.., n stride): the first n values at p[r stride], NaN in the slots between the strides."""
    p = np.full(values.shape[:-1] + (n * stride,), np.nan, np.float64)
    p[..., ::stride] = values[..., :n]
    return p


# ---- the cases: one per op of mobgs_lane_probe --------------------------------------------------------------------------------
class Case:
    """op: the MOBGS_LANE_* name; dtype, T, KI, KO: the launch's layout; inputs: (G, T, KI); expected: (G, T, KO);
    threads: the threads the contract specifies (None: all); span: the threads that must hold one bit pattern (0: none);
    order: the name of the primitive's order_table, if it has one."""

    def __init__(self, op, inputs, expected, threads=None, span=0, order=None, n=0, stride=1, raw_inputs=None):
        self.op, self.inputs, self.expected, self.threads, self.span, self.order = op, inputs, expected, threads, span, order
        self.n, self.stride = n, stride
        self.raw_inputs = inputs if raw_inputs is None else raw_inputs   # what goes to the device
        self.dtype = expected.dtype
        self.G, self.T, self.KO = expected.shape

    def __repr__(self):
        return self.op if not self.n and self.stride == 1 else f"{self.op}-n{self.n}-s{self.stride}"


def _lanewise(op, vectors, fn, span=WAVE, order=None):
    """vectors (G, 64) -> a 1 -> 1 case; fn works with the lane axis last."""
    return Case(op, vectors[:, :, None], fn(vectors)[:, :, None], span=span, order=order)


def _floats(seed, count=8):
    return _draw(np.random.default_rng(seed), (count, WAVE), np.float32)


def _sum_table(dtype, order):
    return np.concatenate([counting(dtype), order_table(order), specials(dtype)])


def _minmax_table(dtype):
    if np.dtype(dtype).kind == "i":
        rng = np.random.default_rng(21)
        return np.concatenate([counting(dtype), specials(dtype), rng.integers(-2**31, 2**31, (8, WAVE)).astype(dtype)])
    return np.concatenate([counting(dtype), specials(dtype), _floats(22)])


@functools.lru_cache(maxsize=None)
def wave_cases():
    f32, f64, i32, u32 = np.float32, np.float64, np.int32, np.uint32
    cases = [
        _lanewise("MOBGS_LANE_WAVE_SUM_F32", _sum_table(f32, "wave_sum_f32"), wave_sum, order="wave_sum_f32"),
        _lanewise("MOBGS_LANE_WAVE_SUM_I32", counting(i32), wave_sum),
        _lanewise("MOBGS_LANE_WAVE_SUM_F64", _sum_table(f64, "wave_sum_f64"), wave_sum, order="wave_sum_f64"),
        _lanewise("MOBGS_LANE_WAVE_MIN_F32", _minmax_table(f32), wave_min),
        _lanewise("MOBGS_LANE_WAVE_MIN_I32", _minmax_table(i32), wave_min),
        _lanewise("MOBGS_LANE_WAVE_MAX_F32", _minmax_table(f32), wave_max),
        _lanewise("MOBGS_LANE_WAVE_MAX_I32", _minmax_table(i32), wave_max),
        _lanewise("MOBGS_LANE_FOLD_MAX_I32", _minmax_table(i32), wave_max),
        _lanewise("MOBGS_LANE_FOLD_ADD_I32", counting(i32), wave_sum),
        _lanewise("MOBGS_LANE_FOLD_ADD_F32", _sum_table(f32, "wave_sum_f32"), wave_sum, order="wave_sum_f32"),
    ]
    lane_index = np.stack([LANES, 1000 + 7 * LANES]).astype(u32)      # the payload is the lane index: out = the lane map
    for op, ctrl in (("XOR1", 0xB1), ("XOR2", 0x4E), ("QUAD_REVERSE", 0x1B), ("HALF_MIRROR", 0x141), ("ROR8", 0x128)):
        cases.append(_lanewise("MOBGS_LANE_DPP_MOV_" + op, lane_index, lambda v, c=ctrl: dpp_mov(v, c), span=0))
    cases.append(_lanewise("MOBGS_LANE_DPP_MOV_XOR4", lane_index, lambda v: dpp_mov(dpp_mov(v, 0x141), 0x1B), span=0))
    steps = np.concatenate([counting(f32), specials(f32), _floats(23)])
    for op, ctrl in (("XOR1", 0xB1), ("XOR2", 0x4E), ("HALF_MIRROR", 0x141), ("ROR8", 0x128), ("ROR4", 0x124)):
        cases.append(_lanewise("MOBGS_LANE_DPP_ADD_" + op, steps, lambda v, c=ctrl: dpp_add(v, c), span=0))
    cases.append(_lanewise("MOBGS_LANE_DPP_ADD_XOR4", steps, dpp_add_xor4, span=0))
    cases += [
        _lanewise("MOBGS_LANE_ROW_ALLREDUCE", _sum_table(f32, "row_allreduce"), row_allreduce, 16, "row_allreduce"),
        _lanewise("MOBGS_LANE_HALF_WAVE_SUM", _sum_table(f32, "half_wave_sum"), half_wave_sum, 32, "half_wave_sum"),
        _lanewise("MOBGS_LANE_WAVE_ALLREDUCE", _sum_table(f32, "wave_allreduce"), wave_allreduce, WAVE, "wave_allreduce"),
    ]
    for nvp in NVPS:
        order = f"wave_reduce_components_{nvp}"
        x = np.concatenate([placement(nvp), order_table(order)])
        y = wave_reduce_components(x.transpose(0, 2, 1)).transpose(0, 2, 1)
        cases.append(Case(f"MOBGS_LANE_REDUCE_COMPONENTS_{nvp}", x, y, span=16, order=order))
    x = np.concatenate([placement(2), order_table("wave_reduce_pair")])
    cases.append(Case("MOBGS_LANE_REDUCE_PAIR", x, wave_reduce_pair(x[:, :, 0], x[:, :, 1])[:, :, None], span=32,
                      order="wave_reduce_pair"))
    cases.append(Case("MOBGS_LANE_WAVE_FENCE", lane_index[:, :, None], wave_fence(lane_index)))
    return cases


def _two_calls(vectors):
    """(2 G, BLOCK) -> (G, BLOCK, 2): consecutive vectors go to the first and the second call of one workgroup."""
    return vectors.reshape(-1, 2, BLOCK).transpose(0, 2, 1)


@functools.lru_cache(maxsize=None)
def block_cases():
    f32, f64 = np.float32, np.float64
    cases = []
    for op, dtype, order, fn, threads in (("MOBGS_LANE_BLOCK_SUM", f64, "block_sum", block_sum, (0,)),
                                          ("MOBGS_LANE_BLOCK_SUM4", f32, "block_sum4", block_sum4, None)):
        count = counting(dtype, BLOCK)
        x = _two_calls(np.concatenate([count, count[::-1], order_table(order), specials(dtype, BLOCK),
                                       specials(dtype, BLOCK)[::-1][1:], count[:1]]))
        y = np.stack([fn(x[:, :, 0]), fn(x[:, :, 1])], axis=-1)
        y = np.broadcast_to(y[:, None, :], x.shape).copy()
        cases.append(Case(op, x, y, threads=threads, span=0 if threads else BLOCK, order=order))
    return cases


def _rows_values(order, per_group):
    """(G, per_group, 2 BLOCK + 3): the order-sensitive vectors, all ones and the row index."""
    n = ROW_COUNTS[-1]
    extra = np.stack([np.ones(n), np.arange(n, dtype=np.float64)] * per_group)
    return np.concatenate([order_table(order), extra]).reshape(-1, per_group, n)


@functools.lru_cache(maxsize=None)
def rows_cases():
    """ROWS_SUM and WAVE_ROWS_SUM at every row count and stride; the inputs are arrays, not per-thread values."""
    cases = []
    for n in ROW_COUNTS:
        for stride in STRIDES:
            v = _rows_values("rows_sum", 2)
            p = strided(v, n, stride)                                       # (G, 2, n stride)
            y = np.broadcast_to(rows_sum(p, n, stride)[:, None, :], (len(p), BLOCK, 2)).copy()
            cases.append(Case("MOBGS_LANE_ROWS_SUM", p, y, threads=(0,), order="rows_sum", n=n, stride=stride,
                              raw_inputs=p.reshape(len(p), -1)))
            v = _rows_values("wave_rows_sum", 1)
            p = strided(v, n, stride)                                       # (G, 1, n stride)
            y = np.broadcast_to(wave_rows_sum(p[:, 0], n, stride)[:, None, None], (len(p), WAVE, 1)).copy()
            cases.append(Case("MOBGS_LANE_WAVE_ROWS_SUM", p, y, span=WAVE, order="wave_rows_sum", n=n, stride=stride,
                              raw_inputs=p.reshape(len(p), -1)))
    return cases


def all_cases():
    return wave_cases() + block_cases() + rows_cases()
