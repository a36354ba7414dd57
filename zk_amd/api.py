"""Python mirror of the reference's public API for the hot path, over the C ABI (include/zk_amd.h).

Same names, argument meaning and error behaviour as the reference crates (paths relative to the reference):
  polynomial::multilinear::evaluation_form::MultiLinearPolynomial   evaluation_form.rs:7-103
  polynomial::product_poly::ProductPoly                             product_poly.rs:7-88
  sumcheck::prover::SumcheckProver<MAX_VAR_DEGREE, F>               prover.rs:9-73
  sumcheck::verifier::SumcheckVerifier<F>                           verifier.rs:9-78
  transcript::Transcript                                            transcript/src/lib.rs:5-35
  fft::{fft, ifft, fft_internal}                                    fft/src/lib.rs:4-46
`Err(&'static str)` becomes ZkError with the same text; misuse the reference panics on becomes ZkError too.
Field elements are numpy uint64 arrays of shape (..., 4): ark-ff's in-memory layout (Montgomery, 4 LE limbs).
Everything computes on the GPU; this module is the test/bench harness and the host side of the sharded prover.
"""
import numpy as np

from ._lib import ZkError, c, check, lib, u8p, u64p

BN254_FR, BLS12_381_FR, BLS12_377_FR = 0, 1, 2
FIELD_NAMES = {BN254_FR: "bn254_fr", BLS12_381_FR: "bls12_381_fr", BLS12_377_FR: "bls12_377_fr"}


def _p(a):
    return a.ctypes.data_as(u64p)


def _elems(x, n=None):
    a = np.ascontiguousarray(x, dtype=np.uint64).reshape(-1, 4)
    if n is not None and a.shape[0] != n:
        raise ValueError(f"expected {n} field elements, got {a.shape[0]}")
    return a


# ---- host-side element helpers (no GPU needed) ---------------------------------------------------------------
def modulus(field):
    out = np.zeros(4, dtype=np.uint64)
    check(lib.zk_field_modulus(field, _p(out)))
    return sum(int(v) << (64 * i) for i, v in enumerate(out))


def two_adicity(field):
    s = c.c_int32()
    check(lib.zk_field_two_adicity(field, c.byref(s)))
    return s.value


def root_of_unity(field, log_n):
    """F::get_root_of_unity(2^log_n) (fft/src/lib.rs:6) as a Montgomery element"""
    out = np.zeros(4, dtype=np.uint64)
    check(lib.zk_field_root_of_unity(field, log_n, _p(out)))
    return out


def fe_from_int(field, v):
    """F::from(v) for any Python int (reduced mod p first)."""
    v %= modulus(field)
    limbs = np.array([(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)
    out = np.zeros(4, dtype=np.uint64)
    check(lib.zk_fe_from_canonical(field, _p(limbs), _p(out)))
    return out


def fe_from_ints(field, vs):
    return np.stack([fe_from_int(field, v) for v in vs]) if len(vs) else np.zeros((0, 4), dtype=np.uint64)


def fe_to_int(field, a):
    a = _elems(a, 1)
    out = np.zeros(4, dtype=np.uint64)
    check(lib.zk_fe_to_canonical(field, _p(a), _p(out)))
    return sum(int(v) << (64 * i) for i, v in enumerate(out))


def fe_to_ints(field, arr):
    arr = _elems(arr)
    return [fe_to_int(field, arr[i]) for i in range(arr.shape[0])]


def mask(n):  # polynomial/src/multilinear/pairing_index.rs:24-26
    """a bit sequence of n ones: mask(1) -> 1, mask(3) -> 0b111"""
    if not 0 <= n < 64:
        raise ZkError(-5, lib.zk_strerror(-5).decode())   # the reference's usize shift overflows here
    return (1 << n) - 1


def index_pair(n_vars, index):  # polynomial/src/multilinear/pairing_index.rs:2-9
    """the (left, right) table indices that partial_evaluate pairs up when it assigns variable `index` (variable 0 = index MSB)"""
    if n_vars < 1 or not 0 <= index < n_vars:
        raise ZkError(-5, lib.zk_strerror(-5).decode())   # u8 underflow in the reference
    pos = n_vars - 1 - index
    out = []
    for j in range(1 << (n_vars - 1)):
        left = ((j >> pos) << (pos + 1)) | (j & mask(pos))
        out.append((left, left | (1 << pos)))
    return out


def keccak256(data: bytes) -> bytes:
    buf = c.create_string_buffer(32)
    check(lib.zk_keccak256(bytes(data), len(data), buf))
    return buf.raw


class Transcript:
    """transcript::Transcript (transcript/src/lib.rs:5-35)."""

    def __init__(self):
        h = c.c_void_p()
        check(lib.zk_transcript_new(c.byref(h)))
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None):
            lib.zk_transcript_free(self._h)
            self._h = None

    def append(self, new_data: bytes):
        check(lib.zk_transcript_append(self._h, bytes(new_data), len(new_data)))

    def sample_challenge(self) -> bytes:
        buf = c.create_string_buffer(32)
        check(lib.zk_transcript_sample_challenge(self._h, buf))
        return buf.raw

    def sample_field_element(self, field):
        out = np.zeros(4, dtype=np.uint64)
        check(lib.zk_transcript_sample_field_element(self._h, field, _p(out)))
        return out

    def sample_n_field_elements(self, field, n):   # transcript/src/lib.rs:32-34
        out = np.zeros((n, 4), dtype=np.uint64)
        check(lib.zk_transcript_sample_n_field_elements(self._h, field, n, _p(out)))
        return out


# ---- device context ------------------------------------------------------------------------------------------
class Context:
    """One device + stream (zk_ctx).  Fails loudly when there is no gfx950 device."""

    def __init__(self, field=BN254_FR, device=0):
        h = c.c_void_p()
        check(lib.zk_ctx_create(field, device, c.byref(h)))
        self._h, self.field, self.device = h, field, device

    def close(self):
        if getattr(self, "_h", None):
            lib.zk_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def synchronize(self):
        check(lib.zk_ctx_synchronize(self._h))

    def set_stream(self, stream_ptr):
        """run on a caller-owned hipStream_t (0 / None = the legacy default stream)"""
        check(lib.zk_ctx_set_stream(self._h, c.c_void_p(stream_ptr or 0)))

    def use_own_stream(self):
        check(lib.zk_ctx_use_own_stream(self._h))

    def trim(self):
        """drop the context's cache of freed device blocks (zk_ctx_trim)"""
        check(lib.zk_ctx_trim(self._h))

    def use_torch_stream(self):
        """share torch's current stream on this device, so kernels and torch.distributed collectives are ordered"""
        import torch

        self.set_stream(torch.cuda.current_stream(self.device).cuda_stream)

    # measurement hooks
    def bench_copy(self, nbytes, reps=10):
        out = c.c_double()
        check(lib.zk_bench_copy(self._h, nbytes, reps, c.byref(out)))
        return out.value

    def bench_modmul(self, iters=2000, variant=0):
        out = c.c_double()
        check(lib.zk_bench_modmul(self._h, variant, iters, c.byref(out)))
        return out.value


def _handles(polys):
    arr = (c.c_void_p * max(len(polys), 1))(*[q._h for q in polys])
    return c.cast(arr, c.POINTER(c.c_void_p)), arr


class MultiLinearPolynomial:
    """Dense MLE table resident in HBM (evaluation_form.rs:7-10)."""

    def __init__(self, ctx, handle):
        self.ctx, self._h = ctx, handle

    # MultiLinearPolynomial::new (evaluation_form.rs:15-27)
    @classmethod
    def new(cls, ctx, n_vars, evaluations):
        ev = _elems(evaluations)
        h = c.c_void_p()
        check(lib.zk_mle_upload(ctx._h, n_vars, _p(ev), ev.shape[0], c.byref(h)))
        return cls(ctx, h)

    @classmethod
    def new_shard(cls, ctx, n_vars, evaluations, world, rank):
        """shard `rank` of `world` of the natural-order table ::new(n_vars, evaluations) would make: {idx : idx mod world == rank},
        local index idx / world (the layout of the sharded prover and NTT); only the shard goes to the device (zk_mle_upload_shard)"""
        ev = _elems(evaluations)
        h = c.c_void_p()
        check(lib.zk_mle_upload_shard(ctx._h, n_vars, _p(ev), ev.shape[0], world, rank, c.byref(h)))
        return cls(ctx, h)

    @classmethod
    def interleave(cls, shards):
        """inverse of split: `world` equal-size shards -> the natural-order table (zk_mle_interleave, on the device)"""
        shards = list(shards)
        if not shards:
            raise ZkError(-20, lib.zk_strerror(-20).decode())
        ptrs, _keep = _handles(shards)
        h = c.c_void_p()
        check(lib.zk_mle_interleave(shards[0].ctx._h, ptrs, len(shards), c.byref(h)))
        return cls(shards[0].ctx, h)

    @classmethod
    def alloc(cls, ctx, n_vars):
        h = c.c_void_p()
        check(lib.zk_mle_alloc(ctx._h, n_vars, c.byref(h)))
        return cls(ctx, h)

    @classmethod
    def random(cls, ctx, n_vars, seed, first_index=0):
        t = cls.alloc(ctx, n_vars)
        check(lib.zk_mle_fill_random(ctx._h, t._h, seed, first_index))
        return t

    def free(self):
        if getattr(self, "_h", None) and getattr(self.ctx, "_h", None):
            lib.zk_mle_free(self.ctx._h, self._h)
        self._h = None

    def __del__(self):
        self.free()

    def clone(self):
        h = c.c_void_p()
        check(lib.zk_mle_clone(self.ctx._h, self._h, c.byref(h)))
        return MultiLinearPolynomial(self.ctx, h)

    def split(self, world):
        """all `world` shards by index mod world, in rank order (zk_mle_split, one pass on the device); self is unchanged"""
        hs = (c.c_void_p * max(int(world), 1))()
        check(lib.zk_mle_split(self.ctx._h, self._h, world, c.cast(hs, c.POINTER(c.c_void_p))))
        return [MultiLinearPolynomial(self.ctx, c.c_void_p(h)) for h in hs[:world]]

    def n_vars(self):
        n = c.c_uint64()
        check(lib.zk_mle_n_vars(self._h, c.byref(n)))
        return n.value

    def device_ptr(self):
        p = c.c_void_p()
        check(lib.zk_mle_device_ptr(self._h, c.byref(p)))
        return p.value

    # partial_evaluate (evaluation_form.rs:40-80)
    def partial_evaluate(self, initial_var, assignments):
        a = _elems(assignments)
        h = c.c_void_p()
        check(lib.zk_mle_partial_evaluate(self.ctx._h, self._h, initial_var, _p(a), a.shape[0], c.byref(h)))
        return MultiLinearPolynomial(self.ctx, h)

    def fold_into(self, r, out):
        r = _elems(r, 1)
        check(lib.zk_mle_fold_into(self.ctx._h, self._h, _p(r), out._h))
        return out

    def bench_fold(self, r, out, reps):
        r = _elems(r, 1)
        ms = c.c_double()
        check(lib.zk_bench_fold(self.ctx._h, self._h, _p(r), out._h, reps, c.byref(ms)))
        return ms.value

    def bench_fold_samples(self, r, out, reps, group=1):
        """launch durations (ms) of `reps` folds: one HIP event every `group` launches, each sample the average inside its group"""
        r = _elems(r, 1)
        ms = np.zeros((reps + group - 1) // group, dtype=np.float64)
        check(lib.zk_bench_fold_samples(self.ctx._h, self._h, _p(r), out._h, reps, group, ms.ctypes.data_as(c.POINTER(c.c_double))))
        return ms

    # evaluate (evaluation_form.rs:83-89)
    def evaluate(self, assignments):
        a = _elems(assignments)
        out = np.zeros(4, dtype=np.uint64)
        check(lib.zk_mle_evaluate(self.ctx._h, self._h, _p(a), a.shape[0], _p(out)))
        return out

    # evaluation_slice (evaluation_form.rs:92-94)
    def evaluation_slice(self):
        out = np.zeros((1 << self.n_vars(), 4), dtype=np.uint64)
        check(lib.zk_mle_download(self.ctx._h, self._h, _p(out)))
        return out

    # to_bytes (evaluation_form.rs:97-103)
    def to_bytes_array(self, out=None):
        """to_bytes (evaluation_form.rs:97-103) into a numpy uint8 array (a fresh one, or `out`): no second host copy"""
        if out is None:
            out = np.empty(32 << self.n_vars(), dtype=np.uint8)
        want = 32 << self.n_vars()   # zk_mle_to_bytes writes exactly this many bytes, on several host threads
        if not isinstance(out, np.ndarray) or out.dtype != np.uint8 or out.size != want:
            raise ValueError(f"to_bytes_array: out must be a numpy uint8 array of {want} bytes")
        if not out.flags["C_CONTIGUOUS"] or not out.flags["WRITEABLE"]:
            raise ValueError("to_bytes_array: out must be C-contiguous and writeable")
        check(lib.zk_mle_to_bytes(self.ctx._h, self._h, out.ctypes.data_as(u8p)))
        return out

    def to_bytes(self):
        return self.to_bytes_array().tobytes()

    # batch inversion and running products (zk_mle_batch_inverse / zk_mle_prefix_product; the reference has none)
    def batch_inverse(self, shift=None, out=None, count_zeros=False):
        """out[i] = 1 / (self[i] + shift), zero where the denominator is zero (no error).  out None: a new table; out=self: in place.
        Returns the table, or (table, zeros) with count_zeros (the only form that waits for the stream)."""
        if out is None:
            out = MultiLinearPolynomial.alloc(self.ctx, self.n_vars())
        sv = None if shift is None else _elems(shift, 1)
        zeros = c.c_uint64()
        check(lib.zk_mle_batch_inverse(self.ctx._h, self._h, None if sv is None else _p(sv), out._h, c.byref(zeros) if count_zeros else None))
        return (out, zeros.value) if count_zeros else out

    def prefix_product(self, inclusive=False, out=None, want_total=False):
        """exclusive: out[0] = 1, out[i] = self[0] ... self[i-1]; inclusive: out[i] = self[0] ... self[i].  out None: a new table;
        out=self: in place.  Returns the table, or (table, product of all elements) with want_total (which waits for the stream)."""
        if out is None:
            out = MultiLinearPolynomial.alloc(self.ctx, self.n_vars())
        total = np.zeros(4, dtype=np.uint64)
        check(lib.zk_mle_prefix_product(self.ctx._h, self._h, 1 if inclusive else 0, out._h, _p(total) if want_total else None))
        return (out, total) if want_total else out

    def bench_batch_inverse(self, out, path=0, reps=20):
        """device ms per call (zk_bench_batch_inverse): path 0 default, 1 one launch, 2 three launches, 3 prefix_product"""
        ms = c.c_double()
        check(lib.zk_bench_batch_inverse(self.ctx._h, self._h, out._h, path, reps, c.byref(ms)))
        return ms.value

    def __eq__(self, other):  # #[derive(PartialEq)] (evaluation_form.rs:4)
        if not isinstance(other, MultiLinearPolynomial):
            return NotImplemented
        if other.ctx is not self.ctx:   # different contexts: compare on the host
            return self.n_vars() == other.n_vars() and np.array_equal(self.evaluation_slice(), other.evaluation_slice())
        eq = c.c_int32()
        check(lib.zk_mle_equal(self.ctx._h, self._h, other._h, c.byref(eq)))
        return bool(eq.value)

    __hash__ = None


class UnivariatePolynomial:
    """Coefficient vector resident in HBM, lowest degree first (univariate_poly.rs:7-12); any length, 0 included."""

    def __init__(self, ctx, handle):
        self.ctx, self._h = ctx, handle

    # UnivariatePolynomial::new (univariate_poly.rs:16-19)
    @classmethod
    def new(cls, ctx, coefficients):
        co = _elems(coefficients)
        h = c.c_void_p()
        check(lib.zk_upoly_upload(ctx._h, _p(co), co.shape[0], c.byref(h)))
        return cls(ctx, h)

    def free(self):
        if getattr(self, "_h", None) and getattr(self.ctx, "_h", None):
            lib.zk_upoly_free(self.ctx._h, self._h)
        self._h = None

    def __del__(self):
        self.free()

    def len(self):
        n = c.c_uint64()
        check(lib.zk_upoly_len(self._h, c.byref(n)))
        return n.value

    # coefficients (univariate_poly.rs:21-23)
    def coefficients(self):
        out = np.zeros((self.len(), 4), dtype=np.uint64)
        check(lib.zk_upoly_download(self.ctx._h, self._h, _p(out)))
        return out

    # evaluate (univariate_poly.rs:29-40)
    def evaluate(self, x):
        xv = _elems(x, 1)
        out = np.zeros(4, dtype=np.uint64)
        check(lib.zk_upoly_evaluate(self.ctx._h, self._h, _p(xv), _p(out)))
        return out

    # Mul for &UnivariatePolynomial (univariate_poly.rs:186-209)
    def __mul__(self, other):
        if not isinstance(other, UnivariatePolynomial):
            return NotImplemented
        h = c.c_void_p()
        check(lib.zk_upoly_mul(self.ctx._h, self._h, other._h, c.byref(h)))
        return UnivariatePolynomial(self.ctx, h)

    # Add for &UnivariatePolynomial (univariate_poly.rs:157-184)
    def __add__(self, other):
        if not isinstance(other, UnivariatePolynomial):
            return NotImplemented
        h = c.c_void_p()
        check(lib.zk_upoly_add(self.ctx._h, self._h, other._h, c.byref(h)))
        return UnivariatePolynomial(self.ctx, h)

    # UnivariatePolynomial::interpolate (univariate_poly.rs:43-49): xs = 0 .. n-1, exactly n coefficients
    @classmethod
    def interpolate(cls, ctx, ys):
        yp = ys if isinstance(ys, UnivariatePolynomial) else cls.new(ctx, ys)
        h = c.c_void_p()
        check(lib.zk_upoly_interpolate(ctx._h, yp._h, c.byref(h)))
        return cls(ctx, h)

    # UnivariatePolynomial::interpolate_xy (univariate_poly.rs:54-80); a repeated x at an index < min(nx, ny) raises ZkError (-11)
    @classmethod
    def interpolate_xy(cls, ctx, xs, ys):
        xp = xs if isinstance(xs, UnivariatePolynomial) else cls.new(ctx, xs)
        yp = ys if isinstance(ys, UnivariatePolynomial) else cls.new(ctx, ys)
        h = c.c_void_p()
        check(lib.zk_upoly_interpolate_xy(ctx._h, xp._h, yp._h, c.byref(h)))
        return cls(ctx, h)

    # evaluate (univariate_poly.rs:29-40) at every point of xs: a device vector of len(xs) values, no host wait
    def evaluate_many(self, xs):
        """xs: a UnivariatePolynomial used as a vector of points, field elements (n x 4 limbs), or a list of Python ints (taken mod p)"""
        if isinstance(xs, UnivariatePolynomial):
            xp = xs
        elif isinstance(xs, (list, tuple)) and all(isinstance(v, int) for v in xs):
            xp = UnivariatePolynomial.new(self.ctx, fe_from_ints(self.ctx.field, [v % modulus(self.ctx.field) for v in xs]))
        else:
            xp = UnivariatePolynomial.new(self.ctx, xs)
        h = c.c_void_p()
        check(lib.zk_upoly_evaluate_many(self.ctx._h, self._h, xp._h, c.byref(h)))
        return UnivariatePolynomial(self.ctx, h)

    # division with remainder (zk_upoly_divrem; the reference has none): lengths fix every shape, nothing is trimmed
    def _divrem(self, other, want_q, want_r):
        if not isinstance(other, UnivariatePolynomial):
            other = UnivariatePolynomial.new(self.ctx, other)
        hq, hr = c.c_void_p(), c.c_void_p()
        check(lib.zk_upoly_divrem(self.ctx._h, self._h, other._h, c.byref(hq) if want_q else None, c.byref(hr) if want_r else None))
        return (UnivariatePolynomial(self.ctx, hq) if want_q else None, UnivariatePolynomial(self.ctx, hr) if want_r else None)

    def divmod(self, other):
        """(q, r) with self = q * other + r: len(q) = len(self) - len(other) + 1 and len(r) = len(other) - 1 (q empty and r a copy of
        self when self is the shorter); the divisor's last coefficient is inverted (zero: ZkError, ZK_ERR_PANIC_INVERSE)"""
        return self._divrem(other, True, True)

    def __divmod__(self, other):
        return self._divrem(other, True, True)

    def __floordiv__(self, other):
        return self._divrem(other, True, False)[0]

    def __mod__(self, other):
        return self._divrem(other, False, True)[1]

    def inverse_series(self, k):
        """the k coefficients of 1 / self mod z^k (zk_upoly_inverse_series); self[0] = 0 or self empty: ZkError, ZK_ERR_PANIC_INVERSE"""
        h = c.c_void_p()
        check(lib.zk_upoly_inverse_series(self.ctx._h, self._h, k, c.byref(h)))
        return UnivariatePolynomial(self.ctx, h)

    def batch_inverse(self, shift=None, count_zeros=False):
        """a new vector of 1 / (self[i] + shift), zero where the denominator is zero (zk_upoly_batch_inverse); any length.
        Returns the vector, or (vector, zeros) with count_zeros (the only form that waits for the stream)."""
        sv = None if shift is None else _elems(shift, 1)
        h, zeros = c.c_void_p(), c.c_uint64()
        check(lib.zk_upoly_batch_inverse(self.ctx._h, self._h, None if sv is None else _p(sv), c.byref(h), c.byref(zeros) if count_zeros else None))
        out = UnivariatePolynomial(self.ctx, h)
        return (out, zeros.value) if count_zeros else out

    def __eq__(self, other):  # #[derive(PartialEq)]: same coefficient vector (trailing zeros count)
        if not isinstance(other, UnivariatePolynomial):
            return NotImplemented
        return self.len() == other.len() and np.array_equal(self.coefficients(), other.coefficients())

    __hash__ = None


def upoly_mul_host(ctx, a, b):
    """value-semantics product of two coefficient vectors (zk_upoly_mul_host): la + lb - 1 elements, empty if either is empty"""
    av, bv = _elems(a), _elems(b)
    n = av.shape[0] + bv.shape[0] - 1 if av.shape[0] and bv.shape[0] else 0
    out = np.zeros((max(n, 1), 4), dtype=np.uint64)
    check(lib.zk_upoly_mul_host(ctx._h, _p(av), av.shape[0], _p(bv), bv.shape[0], _p(out)))
    return out[:n]


def upoly_interpolate_host(ctx, ys, xs=None):
    """value-semantics interpolation: ::interpolate (xs None, n coefficients) or ::interpolate_xy (nx coefficients, empty when
    either input is empty)"""
    yv = _elems(ys)
    if xs is None:
        n = yv.shape[0]
        out = np.zeros((max(n, 1), 4), dtype=np.uint64)
        check(lib.zk_upoly_interpolate_host(ctx._h, _p(yv), n, _p(out)))
        return out[:n]
    xv = _elems(xs)
    n = xv.shape[0] if xv.shape[0] and yv.shape[0] else 0
    out = np.zeros((max(n, 1), 4), dtype=np.uint64)
    check(lib.zk_upoly_interpolate_xy_host(ctx._h, _p(xv), xv.shape[0], _p(yv), yv.shape[0], _p(out)))
    return out[:n]


def upoly_evaluate_many_host(ctx, coeffs, xs):
    """value-semantics multipoint evaluation (zk_upoly_evaluate_many_host): the polynomial's value at every point of xs"""
    cv, xv = _elems(coeffs), _elems(xs)
    n = xv.shape[0]
    out = np.zeros((max(n, 1), 4), dtype=np.uint64)
    check(lib.zk_upoly_evaluate_many_host(ctx._h, _p(cv), cv.shape[0], _p(xv), n, _p(out)))
    return out[:n]


def upoly_divrem_host(ctx, a, b):
    """value-semantics division with remainder (zk_upoly_divrem_host): (q, r) as arrays of len(a) - len(b) + 1 and len(b) - 1 elements
    (0 and len(a) when a is the shorter)"""
    av, bv = _elems(a), _elems(b)
    la, lb = av.shape[0], bv.shape[0]
    lq, lr = (la - lb + 1, lb - 1) if la >= lb else (0, la)
    q = np.zeros((max(lq, 1), 4), dtype=np.uint64)
    r = np.zeros((max(lr, 1), 4), dtype=np.uint64)
    check(lib.zk_upoly_divrem_host(ctx._h, _p(av), la, _p(bv), lb, _p(q), _p(r)))
    return q[:lq], r[:lr]


def batch_inverse_host(ctx, values, shift=None):
    """value-semantics batch inversion (zk_batch_inverse_host): (1 / (values[i] + shift) with zeros left zero, number of zeros)"""
    v = _elems(values)
    n = v.shape[0]
    sv = None if shift is None else _elems(shift, 1)
    out = np.zeros((max(n, 1), 4), dtype=np.uint64)
    zeros = c.c_uint64()
    check(lib.zk_batch_inverse_host(ctx._h, _p(v) if n else None, n, None if sv is None else _p(sv), _p(out) if n else None, c.byref(zeros)))
    return out[:n], zeros.value


class MerkleTree:
    """Binary Keccak-256 Merkle commitment over k tables of 2^n elements, every level resident on the device (zk_merkle; the reference
    has none, tests/merkle_ref.py is the definition): leaf i hashes the 32-byte big-endian canonical images of row i of all columns."""

    def __init__(self, ctx, handle):
        self.ctx, self._h = ctx, handle

    @classmethod
    def commit(cls, columns):
        """stream-ordered, no host wait; the tree does not refer to the columns afterwards"""
        columns = list(columns)
        if not columns:
            raise ZkError(-20, lib.zk_strerror(-20).decode())
        ptrs, _keep = _handles(columns)
        h = c.c_void_p()
        check(lib.zk_merkle_commit(columns[0].ctx._h, ptrs, len(columns), c.byref(h)))
        return cls(columns[0].ctx, h)

    def free(self):
        if getattr(self, "_h", None) and getattr(self.ctx, "_h", None):
            lib.zk_merkle_free(self._h)
        self._h = None

    def __del__(self):
        self.free()

    def n_vars(self):
        out = c.c_uint32()
        check(lib.zk_merkle_n_vars(self._h, c.byref(out)))
        return out.value

    def n_columns(self):
        out = c.c_uint32()
        check(lib.zk_merkle_n_columns(self._h, c.byref(out)))
        return out.value

    def root(self):
        """the 32 bytes of level[n][0]; waits for the stream"""
        buf = np.zeros(32, dtype=np.uint8)
        check(lib.zk_merkle_root(self.ctx._h, self._h, buf.ctypes.data_as(u8p)))
        return buf.tobytes()

    def level(self, d):
        """the 2^(n - d) digests of level d (0 = the leaves) as a (2^(n - d), 32) uint8 array"""
        n = self.n_vars()
        buf = np.zeros((1 << max(n - d, 0), 32), dtype=np.uint8)
        check(lib.zk_merkle_level(self.ctx._h, self._h, d, buf.ctypes.data_as(u8p)))
        return buf

    def open(self, indices, columns=None):
        """(rows, paths) of the rows `indices` (any order, duplicates allowed): paths is (q, n, 32) uint8, the siblings bottom up;
        rows is the (q, k, 4) elements of the given columns (the caller's claim, not re-hashed), or None without columns"""
        idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
        q, n, k = idx.shape[0], self.n_vars(), self.n_columns()
        paths = np.zeros((q, n, 32), dtype=np.uint8)
        rows = None
        ptrs, n_cols = None, 0
        if columns is not None:
            columns = list(columns)
            ptrs, _keep = _handles(columns)
            n_cols = len(columns)
            rows = np.zeros((q, k, 4), dtype=np.uint64)
        check(lib.zk_merkle_open(self.ctx._h, self._h, ptrs, n_cols, idx.ctypes.data_as(u64p), q, None if rows is None else _p(rows),
                                 paths.ctypes.data_as(u8p)))
        return rows, paths

    @staticmethod
    def bench(columns, path=0, reps=5):
        """device ms per build of the tree (zk_bench_merkle): path 0 default, 1 fused sub-tree stages, 2 one launch per level"""
        columns = list(columns)
        ptrs, _keep = _handles(columns)
        ms = c.c_double()
        check(lib.zk_bench_merkle(columns[0].ctx._h, ptrs, len(columns), path, reps, c.byref(ms)))
        return ms.value


def merkle_verify(field, root, n_vars, index, row, path):
    """host only (zk_merkle_verify_host): does `path` (n_vars digests, bottom up) lead from the leaf of `row` (its k elements) at `index`
    to `root`?"""
    rv = _elems(row)
    rt = np.frombuffer(bytes(root), dtype=np.uint8)
    pv = np.frombuffer(bytes(path), dtype=np.uint8) if isinstance(path, (bytes, bytearray)) else np.ascontiguousarray(path, dtype=np.uint8).reshape(-1)
    if rt.shape[0] != 32 or pv.shape[0] != 32 * n_vars:
        raise ZkError(-20, lib.zk_strerror(-20).decode())
    ok = c.c_int32()
    check(lib.zk_merkle_verify_host(field, rt.ctypes.data_as(u8p), n_vars, rv.shape[0], index, _p(rv), pv.ctypes.data_as(u8p) if n_vars else None,
                                    c.byref(ok)))
    return bool(ok.value)


# ---- FRI low-degree proofs (zk_fri_*; the reference has none, tests/fri_ref.py is the definition) ------------------------------------
def fri_lde(poly, log_n, shift):
    """the evaluations of `poly` (a UnivariatePolynomial of at most 2^log_n coefficients) over shift * <root_of_unity(2^log_n)> in
    natural order, as a new MultiLinearPolynomial of log_n variables"""
    sv = _elems(shift, 1)
    h = c.c_void_p()
    check(lib.zk_fri_lde(poly.ctx._h, poly._h, log_n, _p(sv), c.byref(h)))
    return MultiLinearPolynomial(poly.ctx, h)


def fri_fold(layer, log_arity, shift, beta, out=None):
    """fold `layer` (2^n evaluations over the coset of `shift`) by 2^log_arity at the challenge `beta` into `out` (a table of
    n - log_arity variables, allocated when not given); `layer` is left intact"""
    sv, bv = _elems(shift, 1), _elems(beta, 1)
    if out is None:
        n = layer.n_vars()
        if n < log_arity:
            raise ZkError(-1, lib.zk_strerror(-1).decode())
        out = MultiLinearPolynomial.alloc(layer.ctx, n - log_arity)
    check(lib.zk_fri_fold(layer.ctx._h, layer._h, log_arity, _p(sv), _p(bv), out._h))
    return out


def fri_proof_bytes(log_degree, log_blowup, log_arity, log_final, n_queries):
    n = c.c_uint64()
    check(lib.zk_fri_proof_bytes(log_degree, log_blowup, log_arity, log_final, n_queries, c.byref(n)))
    return n.value


def fri_prove(poly, log_degree, log_blowup, log_arity, log_final, n_queries, shift, seed):
    """the proof bytes that `poly` has fewer than 2^log_degree + 1 coefficients: R = (log_degree - log_final) / log_arity roots, the
    2^log_final final coefficients, and per query and round the opened row and its path"""
    sv = _elems(shift, 1)
    sd = np.frombuffer(bytes(seed), dtype=np.uint8)
    if sd.shape[0] != 32:
        raise ZkError(-20, lib.zk_strerror(-20).decode())
    out = np.zeros(fri_proof_bytes(log_degree, log_blowup, log_arity, log_final, n_queries), dtype=np.uint8)
    check(lib.zk_fri_prove(poly.ctx._h, poly._h, log_degree, log_blowup, log_arity, log_final, n_queries, _p(sv), sd.ctypes.data_as(u8p),
                           out.ctypes.data_as(u8p)))
    return out.tobytes()


def fri_verify(field, proof, log_degree, log_blowup, log_arity, log_final, n_queries, shift, seed):
    """host only (zk_fri_verify_host): does `proof` show a polynomial below the degree bound under these parameters?"""
    sv = _elems(shift, 1)
    sd = np.frombuffer(bytes(seed), dtype=np.uint8)
    pv = np.frombuffer(bytes(proof), dtype=np.uint8)
    if sd.shape[0] != 32 or pv.shape[0] == 0:
        raise ZkError(-20, lib.zk_strerror(-20).decode())
    ok = c.c_int32()
    check(lib.zk_fri_verify_host(field, log_degree, log_blowup, log_arity, log_final, n_queries, _p(sv), sd.ctypes.data_as(u8p),
                                 pv.ctypes.data_as(u8p), pv.shape[0], c.byref(ok)))
    return bool(ok.value)


def bench_fri_fold(layer, log_arity, out, path=0, reps=5):
    """device ms per fold (zk_bench_fri_fold): path 0 default, 1 the fused kernel, 2 log_arity binary launches"""
    ms = c.c_double()
    check(lib.zk_bench_fri_fold(layer.ctx._h, layer._h, log_arity, out._h, path, reps, c.byref(ms)))
    return ms.value


# ---- FRI polynomial commitment (zk_pcs_*, zk_deep_quotient; the reference has none, tests/pcs_ref.py is the definition) ---------------
def _bad_arg():
    return ZkError(-20, lib.zk_strerror(-20).decode())


def deep_quotient(columns, shift, z, values, alpha, out=None):
    """out[i] = (sum_c alpha^c (columns[c][i] - values[c])) / (shift w^i - z) over the columns' coset (zk_deep_quotient); `out` is
    allocated when not given; stream-ordered, the columns are left intact"""
    columns = list(columns)
    if not columns:
        raise _bad_arg()
    sv, zv, av, yv = _elems(shift, 1), _elems(z, 1), _elems(alpha, 1), _elems(values)
    if yv.shape[0] != len(columns):
        raise _bad_arg()
    if out is None:
        out = MultiLinearPolynomial.alloc(columns[0].ctx, columns[0].n_vars())
    ptrs, _keep = _handles(columns)
    check(lib.zk_deep_quotient(columns[0].ctx._h, ptrs, len(columns), _p(sv), _p(zv), _p(yv), _p(av), out._h))
    return out


def bench_deep_quotient(columns, out, reps=5):
    """device ms per quotient (zk_bench_deep_quotient)"""
    columns = list(columns)
    ptrs, _keep = _handles(columns)
    ms = c.c_double()
    check(lib.zk_bench_deep_quotient(columns[0].ctx._h, ptrs, len(columns), out._h, reps, c.byref(ms)))
    return ms.value


def pcs_proof_bytes(k, log_degree, log_blowup, log_arity, log_final, n_queries):
    n = c.c_uint64()
    check(lib.zk_pcs_proof_bytes(k, log_degree, log_blowup, log_arity, log_final, n_queries, c.byref(n)))
    return n.value


class PolyCommitment:
    """One commitment to k univariate polynomials (zk_pcs): their coset LDEs, the Merkle tree over them in FRI's row layout and a copy
    of the coefficients stay on the device, so that it can be opened at any number of points, one after another."""

    def __init__(self, ctx, handle, log_degree, log_blowup, log_arity, shift):
        self.ctx, self._h = ctx, handle
        self.log_degree, self.log_blowup, self.log_arity, self.shift = log_degree, log_blowup, log_arity, shift

    @classmethod
    def commit(cls, polys, log_degree, log_blowup, log_arity, shift):
        polys = list(polys)
        if not polys:
            raise _bad_arg()
        sv = _elems(shift, 1)
        ptrs, _keep = _handles(polys)
        h = c.c_void_p()
        check(lib.zk_pcs_commit(polys[0].ctx._h, ptrs, len(polys), log_degree, log_blowup, log_arity, _p(sv), c.byref(h)))
        return cls(polys[0].ctx, h, log_degree, log_blowup, log_arity, sv.copy())

    def free(self):
        if getattr(self, "_h", None) and getattr(self.ctx, "_h", None):
            lib.zk_pcs_free(self._h)
        self._h = None

    def __del__(self):
        self.free()

    def n_polys(self):
        out = c.c_uint32()
        check(lib.zk_pcs_n_polys(self._h, c.byref(out)))
        return out.value

    def root(self):
        """the commitment: 32 bytes; waits for the stream"""
        buf = np.zeros(32, dtype=np.uint8)
        check(lib.zk_pcs_root(self.ctx._h, self._h, buf.ctypes.data_as(u8p)))
        return buf.tobytes()

    def open(self, z, log_final, n_queries, seed):
        """(values, proof): the k values f_c(z) as a (k, 4) array and the proof bytes that they are right"""
        zv = _elems(z, 1)
        sd = np.frombuffer(bytes(seed), dtype=np.uint8)
        if sd.shape[0] != 32:
            raise _bad_arg()
        k = self.n_polys()
        values = np.zeros((k, 4), dtype=np.uint64)
        proof = np.zeros(pcs_proof_bytes(k, self.log_degree, self.log_blowup, self.log_arity, log_final, n_queries), dtype=np.uint8)
        check(lib.zk_pcs_open(self.ctx._h, self._h, _p(zv), log_final, n_queries, sd.ctypes.data_as(u8p), _p(values), proof.ctypes.data_as(u8p)))
        return values, proof.tobytes()


def pcs_verify(field, root, z, values, proof, log_degree, log_blowup, log_arity, log_final, n_queries, shift, seed):
    """host only (zk_pcs_verify_host): does `proof` show that the k polynomials committed to by `root` take `values` at `z`?"""
    sv, zv, yv = _elems(shift, 1), _elems(z, 1), _elems(values)
    sd, rt, pv = (np.frombuffer(bytes(x), dtype=np.uint8) for x in (seed, root, proof))
    if sd.shape[0] != 32 or rt.shape[0] != 32 or pv.shape[0] == 0 or yv.shape[0] == 0:
        raise _bad_arg()
    ok = c.c_int32()
    check(lib.zk_pcs_verify_host(field, yv.shape[0], log_degree, log_blowup, log_arity, log_final, n_queries, _p(sv), sd.ctypes.data_as(u8p),
                                 rt.ctypes.data_as(u8p), _p(zv), _p(yv), pv.ctypes.data_as(u8p), pv.shape[0], c.byref(ok)))
    return bool(ok.value)


# ---- multilinear polynomial commitment (zk_mlpcs_*, zk_mle_eq_sums; the reference has none, tests/mlpcs_ref.py is the definition) -----
def mlpcs_proof_bytes(n_vars, log_blowup, log_final, n_queries):
    n = c.c_uint64()
    check(lib.zk_mlpcs_proof_bytes(n_vars, log_blowup, log_final, n_queries, c.byref(n)))
    return n.value


class MultilinearCommitment:
    """One commitment to a table (zk_mlpcs): a copy of the table, the coset LDE of its coefficient form and the Merkle tree over it stay
    on the device, so that it can be opened at any number of points, one after another."""

    def __init__(self, ctx, handle, log_blowup, shift):
        self.ctx, self._h = ctx, handle
        self.log_blowup, self.shift = log_blowup, shift

    @classmethod
    def commit(cls, table, log_blowup, shift):
        sv = _elems(shift, 1)
        h = c.c_void_p()
        check(lib.zk_mlpcs_commit(table.ctx._h, table._h, log_blowup, _p(sv), c.byref(h)))
        return cls(table.ctx, h, log_blowup, sv.copy())

    def free(self):
        if getattr(self, "_h", None) and getattr(self.ctx, "_h", None):
            lib.zk_mlpcs_free(self._h)
        self._h = None

    def __del__(self):
        self.free()

    def n_vars(self):
        out = c.c_uint32()
        check(lib.zk_mlpcs_n_vars(self._h, c.byref(out)))
        return out.value

    def root(self):
        """the commitment: 32 bytes; waits for the stream"""
        buf = np.zeros(32, dtype=np.uint8)
        check(lib.zk_mlpcs_root(self.ctx._h, self._h, buf.ctypes.data_as(u8p)))
        return buf.tobytes()

    def open(self, point, log_final, n_queries, seed):
        """(value, proof): t(point) as 4 limbs and the proof bytes that it is right"""
        pv = _elems(point)
        sd = np.frombuffer(bytes(seed), dtype=np.uint8)
        if sd.shape[0] != 32:
            raise _bad_arg()
        value = np.zeros(4, dtype=np.uint64)
        proof = np.zeros(mlpcs_proof_bytes(self.n_vars(), self.log_blowup, log_final, n_queries), dtype=np.uint8)
        check(lib.zk_mlpcs_open(self.ctx._h, self._h, _p(pv), pv.shape[0], log_final, n_queries, sd.ctypes.data_as(u8p), _p(value),
                                proof.ctypes.data_as(u8p)))
        return value, proof.tobytes()


def mlpcs_verify(field, root, point, value, proof, log_blowup, log_final, n_queries, shift, seed):
    """host only (zk_mlpcs_verify_host): does `proof` show that the table committed to by `root` takes `value` at `point`?"""
    sv, pt, vv = _elems(shift, 1), _elems(point), _elems(value, 1)
    sd, rt, pv = (np.frombuffer(bytes(x), dtype=np.uint8) for x in (seed, root, proof))
    if sd.shape[0] != 32 or rt.shape[0] != 32 or pv.shape[0] == 0 or pt.shape[0] == 0:
        raise _bad_arg()
    ok = c.c_int32()
    check(lib.zk_mlpcs_verify_host(field, pt.shape[0], log_blowup, log_final, n_queries, _p(sv), sd.ctypes.data_as(u8p), rt.ctypes.data_as(u8p),
                                   _p(pt), _p(vv), pv.ctypes.data_as(u8p), pv.shape[0], c.byref(ok)))
    return bool(ok.value)


def eq_sums(table, tail):
    """(2, 4) limbs: S_X = sum_x' table[X 2^(n-1) + x'] eq(x', tail), X = 0, 1 (zk_mle_eq_sums); tail: n_vars - 1 elements"""
    tv = _elems(tail) if len(tail) else np.zeros((0, 4), dtype=np.uint64)
    if tv.shape[0] + 1 != table.n_vars():
        raise _bad_arg()
    out = np.zeros((2, 4), dtype=np.uint64)
    check(lib.zk_mle_eq_sums(table.ctx._h, table._h, _p(tv) if tv.shape[0] else None, _p(out)))
    return out


def bench_mlpcs_round(table, path=0, reps=5):
    """device ms of the sumcheck side of one opening (zk_bench_mlpcs_round): path 0 default, 1 the fused round kernel, 2 the eq table route"""
    ms = c.c_double()
    check(lib.zk_bench_mlpcs_round(table.ctx._h, table._h, path, reps, c.byref(ms)))
    return ms.value


# ---- batch multilinear commitment (zk_mlbatch_*, zk_mle_lincomb, zk_mle_eq_sums_many; tests/mlbatch_ref.py is the definition) ----------
def mlbatch_proof_bytes(n_vars, n_tables, n_points, log_blowup, log_final, n_queries):
    n = c.c_uint64()
    check(lib.zk_mlbatch_proof_bytes(n_vars, n_tables, n_points, log_blowup, log_final, n_queries, c.byref(n)))
    return n.value


class MultilinearBatchCommitment:
    """One commitment to k tables of one size (zk_mlbatch): copies of the tables, their layers and ONE Merkle tree over all of them stay
    on the device; every opening shows all k tables at m points with one proof.  Tables of another size go into another commitment."""

    def __init__(self, ctx, handle, log_blowup, shift):
        self.ctx, self._h = ctx, handle
        self.log_blowup, self.shift = log_blowup, shift

    @classmethod
    def commit(cls, tables, log_blowup, shift):
        tables = list(tables)
        if not tables:
            raise _bad_arg()
        sv = _elems(shift, 1)
        ptr, _keep = _handles(tables)
        h = c.c_void_p()
        check(lib.zk_mlbatch_commit(tables[0].ctx._h, ptr, len(tables), log_blowup, _p(sv), c.byref(h)))
        return cls(tables[0].ctx, h, log_blowup, sv.copy())

    def free(self):
        if getattr(self, "_h", None) and getattr(self.ctx, "_h", None):
            lib.zk_mlbatch_free(self._h)
        self._h = None

    def __del__(self):
        self.free()

    def n_vars(self):
        out = c.c_uint32()
        check(lib.zk_mlbatch_n_vars(self._h, c.byref(out)))
        return out.value

    def n_tables(self):
        out = c.c_uint32()
        check(lib.zk_mlbatch_n_tables(self._h, c.byref(out)))
        return out.value

    def root(self):
        """the commitment: 32 bytes; waits for the stream"""
        buf = np.zeros(32, dtype=np.uint8)
        check(lib.zk_mlbatch_root(self.ctx._h, self._h, buf.ctypes.data_as(u8p)))
        return buf.tobytes()

    def open(self, points, log_final, n_queries, seed):
        """(values, proof): points of shape (m, n_vars, 4); values[j][c] = t_c(points[j]) as (m, k, 4) limbs and the one proof of all of them"""
        n = self.n_vars()
        pv = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 4)
        sd = np.frombuffer(bytes(seed), dtype=np.uint8)
        if sd.shape[0] != 32 or pv.shape[0] == 0 or pv.shape[0] % n:
            raise _bad_arg()
        m, k = pv.shape[0] // n, self.n_tables()
        values = np.zeros((m, k, 4), dtype=np.uint64)
        proof = np.zeros(mlbatch_proof_bytes(n, k, m, self.log_blowup, log_final, n_queries), dtype=np.uint8)
        check(lib.zk_mlbatch_open(self.ctx._h, self._h, _p(pv), m, log_final, n_queries, sd.ctypes.data_as(u8p), _p(values), proof.ctypes.data_as(u8p)))
        return values, proof.tobytes()


def mlbatch_verify(field, root, points, values, proof, log_blowup, log_final, n_queries, shift, seed):
    """host only (zk_mlbatch_verify_host): does `proof` show that the k tables committed to by `root` take values[j][c] at points[j]?
    points: (m, n_vars, 4), values: (m, k, 4)"""
    pt, vv = np.ascontiguousarray(points, dtype=np.uint64), np.ascontiguousarray(values, dtype=np.uint64)
    sv = _elems(shift, 1)
    sd, rt, pv = (np.frombuffer(bytes(x), dtype=np.uint8) for x in (seed, root, proof))
    if pt.ndim != 3 or vv.ndim != 3 or pt.shape[0] != vv.shape[0] or pt.shape[2] != 4 or vv.shape[2] != 4 or 0 in pt.shape or 0 in vv.shape:
        raise _bad_arg()
    if sd.shape[0] != 32 or rt.shape[0] != 32 or pv.shape[0] == 0:
        raise _bad_arg()
    ok = c.c_int32()
    check(lib.zk_mlbatch_verify_host(field, pt.shape[1], vv.shape[1], pt.shape[0], log_blowup, log_final, n_queries, _p(sv), sd.ctypes.data_as(u8p),
                                     rt.ctypes.data_as(u8p), _p(pt), _p(vv), pv.ctypes.data_as(u8p), pv.shape[0], c.byref(ok)))
    return bool(ok.value)


def lincomb(tables, coeffs):
    """a new table sum_c coeffs[c] tables[c] (zk_mle_lincomb); the sources are left intact"""
    tables = list(tables)
    if not tables:
        raise _bad_arg()
    cv = _elems(coeffs, len(tables))
    out = MultiLinearPolynomial.alloc(tables[0].ctx, tables[0].n_vars())
    ptr, _keep = _handles(tables)
    check(lib.zk_mle_lincomb(tables[0].ctx._h, ptr, len(tables), _p(cv), out._h))
    return out


def eq_sums_many(table, tails):
    """(m, 2, 4) limbs: zk_mle_eq_sums at m tails in passes of several points over the table; tails: (m, n_vars - 1, 4)"""
    n = table.n_vars()
    tv = np.ascontiguousarray(tails, dtype=np.uint64)
    if tv.ndim != 3 or tv.shape[0] == 0 or tv.shape[1] != n - 1 or tv.shape[2] != 4:
        raise _bad_arg()
    out = np.zeros((tv.shape[0], 2, 4), dtype=np.uint64)
    check(lib.zk_mle_eq_sums_many(table.ctx._h, table._h, _p(tv) if tv.size else None, tv.shape[0], _p(out)))
    return out


def bench_mlbatch(commitment, n_points=1, path=0, reps=5):
    """device ms (zk_bench_mlbatch): path 0 the device work of one opening at n_points points, 1 the fused combine-and-fold, 2 its unfused
    counterpart, 3 one round at POINTS_PER_PASS points in one pass, 4 the same in single-point passes"""
    ms = c.c_double()
    check(lib.zk_bench_mlbatch(commitment.ctx._h, commitment._h, n_points, path, reps, c.byref(ms)))
    return ms.value


# ---- grand-product argument (zk_mle_product_tree, zk_gprod_*; the reference has none, tests/gprod_ref.py is the definition) -----------
def gprod_proof_bytes(n_vars):
    n = c.c_uint64()
    check(lib.zk_gprod_proof_bytes(n_vars, c.byref(n)))
    return n.value


def _shift_arg(shift):
    return None if shift is None else _elems(shift, 1)


def product_tree(table, shift=None):
    """the product tree over table + shift as a new table in heap order (zk_mle_product_tree): out[0] = 1, out[2^j + i] = V_j[i], so
    out[1] is the product of all entries.  Stream-ordered, no host wait."""
    sv = _shift_arg(shift)
    h = c.c_void_p()
    check(lib.zk_mle_product_tree(table.ctx._h, table._h, None if sv is None else _p(sv), c.byref(h)))
    return MultiLinearPolynomial(table.ctx, h)


def grand_product_prove(table, seed, shift=None):
    """(product, proof, point, claim) of zk_gprod_prove: product = prod_i (table[i] + shift) as 4 limbs, the proof bytes, and the claim
    table(point) = claim the verifier will be left with (point: (n_vars, 4) limbs).  The seed must bind the table (a commitment's root)."""
    sv = _shift_arg(shift)
    sd = np.frombuffer(bytes(seed), dtype=np.uint8)
    if sd.shape[0] != 32:
        raise _bad_arg()
    n = table.n_vars()
    product, claim = np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    point = np.zeros((max(n, 1), 4), dtype=np.uint64)
    proof = np.zeros(gprod_proof_bytes(n), dtype=np.uint8)
    check(lib.zk_gprod_prove(table.ctx._h, table._h, None if sv is None else _p(sv), sd.ctypes.data_as(u8p), _p(product),
                             proof.ctypes.data_as(u8p), _p(point), _p(claim)))
    return product, proof.tobytes(), point, claim


def grand_product_verify(field, n_vars, seed, product, proof, shift=None):
    """host only (zk_gprod_verify_host): (point, claim) -- what is left to check is table(point) == claim -- or None when the proof is
    rejected"""
    sv, pv = _shift_arg(shift), _elems(product, 1)
    sd, pf = (np.frombuffer(bytes(x), dtype=np.uint8) for x in (seed, proof))
    if sd.shape[0] != 32 or pf.shape[0] == 0:
        raise _bad_arg()
    point, claim, ok = np.zeros((max(n_vars, 1), 4), dtype=np.uint64), np.zeros(4, dtype=np.uint64), c.c_int32()
    check(lib.zk_gprod_verify_host(field, n_vars, None if sv is None else _p(sv), sd.ctypes.data_as(u8p), _p(pv), pf.ctypes.data_as(u8p),
                                   pf.shape[0], _p(point), _p(claim), c.byref(ok)))
    return (point, claim) if ok.value else None


def grand_product_verify_table(table, seed, product, proof, shift=None):
    """grand_product_verify plus the evaluation it leaves open, for a verifier that holds the table: True when both hold"""
    got = grand_product_verify(table.ctx.field, table.n_vars(), seed, product, proof, shift)
    return got is not None and bool(np.array_equal(table.evaluate(got[0]), got[1]))


def bench_gprod(table, path=0, reps=5):
    """device ms (zk_bench_gprod): path 0 the product tree on the default route, 1 one level per launch, 2 the whole proof"""
    ms = c.c_double()
    check(lib.zk_bench_gprod(table.ctx._h, table._h, path, reps, c.byref(ms)))
    return ms.value


# ---- zerocheck argument (zk_gate_*, zk_zerocheck_*, zk_mle_gate_sums; the reference has none, tests/zerocheck_ref.py is the definition) --
class Gate:
    """G(x_0 .. x_{k-1}) = sum_i coeff_i prod_{f in cols_i} x_f (zk_gate_create): terms = [(coeff_int, (cols...)), ...]; a repeated
    column is a power, () a constant.  A host object: it needs no context.  A coefficient is any Python int, reduced mod p."""

    def __init__(self, field, k, terms):
        terms = [(int(cf), tuple(int(f) for f in cols)) for cf, cols in terms]
        self.field, self.k, self.terms = field, int(k), terms
        coeffs = fe_from_ints(field, [cf for cf, _ in terms]) if terms else np.zeros((1, 4), dtype=np.uint64)
        lens = np.array([len(cols) for _, cols in terms] or [0], dtype=np.uint32)
        flat = np.array([f for _, cols in terms for f in cols] or [0], dtype=np.uint32)
        u32p = c.POINTER(c.c_uint32)
        h = c.c_void_p()
        check(lib.zk_gate_create(field, self.k, len(terms), _p(np.ascontiguousarray(coeffs)), lens.ctypes.data_as(u32p), flat.ctypes.data_as(u32p),
                                 c.byref(h)))
        self._h = h

    def degree(self):
        d = c.c_uint32()
        check(lib.zk_gate_degree(self._h, c.byref(d)))
        return d.value

    def n_columns(self):
        k = c.c_uint32()
        check(lib.zk_gate_n_columns(self._h, c.byref(k)))
        return k.value

    def free(self):
        if self._h:
            lib.zk_gate_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def zerocheck_proof_bytes(gate, n_vars):
    n = c.c_uint64()
    check(lib.zk_zerocheck_proof_bytes(gate._h, n_vars, c.byref(n)))
    return n.value


def zerocheck_prove(tables, gate, seed):
    """(proof, point, claims) of zk_zerocheck_prove: gate(tables[0][i], .., tables[k-1][i]) = 0 on every row; the verifier is left with
    tables[c](point) = claims[c] (point: (n_vars, 4) limbs, claims: (k, 4)), which one batch opening discharges.  The seed must bind the
    tables (their batch commitment's root).  The prover does not check the statement."""
    sd = np.frombuffer(bytes(seed), dtype=np.uint8)
    if sd.shape[0] != 32 or len(tables) != gate.k:
        raise _bad_arg()
    n = tables[0].n_vars()
    point, claims = np.zeros((max(n, 1), 4), dtype=np.uint64), np.zeros((gate.k, 4), dtype=np.uint64)
    proof = np.zeros(zerocheck_proof_bytes(gate, n), dtype=np.uint8)
    arr, _keep = _handles(tables)
    check(lib.zk_zerocheck_prove(tables[0].ctx._h, arr, gate._h, sd.ctypes.data_as(u8p), proof.ctypes.data_as(u8p), _p(point), _p(claims)))
    return proof.tobytes(), point, claims


def zerocheck_verify(gate, n_vars, seed, proof):
    """host only (zk_zerocheck_verify_host): (point, claims) -- what is left to check is column c at point == claims[c] -- or None when
    the proof is rejected"""
    sd, pf = (np.frombuffer(bytes(x), dtype=np.uint8) for x in (seed, proof))
    if sd.shape[0] != 32 or pf.shape[0] == 0:
        raise _bad_arg()
    point, claims, ok = np.zeros((max(n_vars, 1), 4), dtype=np.uint64), np.zeros((gate.k, 4), dtype=np.uint64), c.c_int32()
    check(lib.zk_zerocheck_verify_host(gate._h, n_vars, sd.ctypes.data_as(u8p), pf.ctypes.data_as(u8p), pf.shape[0], _p(point), _p(claims),
                                       c.byref(ok)))
    return (point, claims) if ok.value else None


def gate_sums(tables, gate, tail):
    """(d + 1, 4) limbs: sum_x' eq(x', tail) gate(tables(X, x')) at X = 0 .. d (zk_mle_gate_sums), the tables as they are; tail: the
    n_vars - 1 elements, anything empty for n_vars = 1"""
    if len(tables) != gate.k:
        raise _bad_arg()
    n = tables[0].n_vars()
    tv = _elems(tail, n - 1) if n > 1 else None
    out = np.zeros((gate.degree() + 1, 4), dtype=np.uint64)
    arr, _keep = _handles(tables)
    check(lib.zk_mle_gate_sums(tables[0].ctx._h, arr, gate._h, None if tv is None else _p(tv), _p(out)))
    return out


def bench_zerocheck(tables, gate, path=0, reps=5):
    """device ms (zk_bench_zerocheck): path 0 the whole proof, 1 the round-0 launch, 2 the round-1 launch (fold joined to the sums)"""
    if len(tables) != gate.k:
        raise _bad_arg()
    ms = c.c_double()
    arr, _keep = _handles(tables)
    check(lib.zk_bench_zerocheck(tables[0].ctx._h, arr, gate._h, path, reps, c.byref(ms)))
    return ms.value


# ---- wiring (copy-constraint) permutation argument (zk_mle_perm_fingerprint, zk_perm_*; the reference has none, tests/perm_ref.py is the definition)
def perm_proof_bytes(n_vars, k):
    n = c.c_uint64()
    check(lib.zk_perm_proof_bytes(n_vars, k, c.byref(n)))
    return n.value


def wiring_sigma(classes):
    """host helper: classes is a (k, 2^n) integer array of copy-class ids (cells of one id must hold one value); returns the (k, 2^n)
    uint64 array of labels sigma_c[i] that wires every class's cells, in label order (c 2^n + i), into one cycle -- a permutation of the
    labels 0 .. k 2^n - 1.  As field elements (fe_from_ints), its rows are the sigma columns of permutation_prove."""
    cl = np.asarray(classes)
    if cl.ndim != 2 or cl.size == 0:
        raise _bad_arg()
    flat = cl.reshape(-1)
    order = np.argsort(flat, kind="stable")   # labels grouped by class, ascending inside a class
    ids = flat[order]
    first = np.ones(ids.shape[0], dtype=bool)
    first[1:] = ids[1:] != ids[:-1]
    start = np.maximum.accumulate(np.where(first, np.arange(ids.shape[0]), 0))   # where each cell's class begins
    last = np.ones(ids.shape[0], dtype=bool)
    last[:-1] = first[1:]
    nxt = np.where(last, order[start], np.roll(order, -1))
    sigma = np.zeros(flat.shape[0], dtype=np.uint64)
    sigma[order] = nxt.astype(np.uint64)
    return sigma.reshape(cl.shape)


def _perm_args(w, sigma, beta, gamma):
    w, sigma = list(w), list(sigma)
    if not w or len(w) != len(sigma):
        raise _bad_arg()
    return w, sigma, _elems(beta, 1), _elems(gamma, 1)


def perm_fingerprint(w, sigma, beta, gamma):
    """the fingerprint table F of n + kappa + 1 variables as a new table (zk_mle_perm_fingerprint): F[2v] = w_c[i] + beta v + gamma,
    F[2v + 1] = w_c[i] + beta sigma_c[i] + gamma for v = c 2^n + i, ones in the padding columns.  Stream-ordered, no host wait."""
    w, sigma, bv, gv = _perm_args(w, sigma, beta, gamma)
    wp, _k1 = _handles(w)
    sp, _k2 = _handles(sigma)
    h = c.c_void_p()
    check(lib.zk_mle_perm_fingerprint(w[0].ctx._h, wp, sp, len(w), _p(bv), _p(gv), c.byref(h)))
    return MultiLinearPolynomial(w[0].ctx, h)


def permutation_prove(w, sigma, beta, gamma, seed):
    """(proof, point, claims) of zk_perm_prove: the witness columns w satisfy the wiring sigma (sigma_c[i] = the label of the cell that
    (c, i) is wired to); the verifier is left with w[c](point) = claims[c], sigma[c](point) = claims[k + c] (point: (n_vars, 4) limbs,
    claims: (2 k, 4)), which one batch opening discharges.  The seed must bind the commitments of w and sigma, and beta, gamma must be
    drawn after that.  The prover does not check the statement."""
    w, sigma, bv, gv = _perm_args(w, sigma, beta, gamma)
    sd = np.frombuffer(bytes(seed), dtype=np.uint8)
    if sd.shape[0] != 32:
        raise _bad_arg()
    n, k = w[0].n_vars(), len(w)
    point, claims = np.zeros((max(n, 1), 4), dtype=np.uint64), np.zeros((2 * k, 4), dtype=np.uint64)
    proof = np.zeros(perm_proof_bytes(n, k), dtype=np.uint8)
    wp, _k1 = _handles(w)
    sp, _k2 = _handles(sigma)
    check(lib.zk_perm_prove(w[0].ctx._h, wp, sp, k, _p(bv), _p(gv), sd.ctypes.data_as(u8p), proof.ctypes.data_as(u8p), _p(point), _p(claims)))
    return proof.tobytes(), point, claims


def permutation_verify(field, n_vars, k, beta, gamma, seed, proof):
    """host only (zk_perm_verify_host): (point, claims) -- what is left to check is w[c](point) == claims[c] and sigma[c](point) ==
    claims[k + c] -- or None when the proof is rejected"""
    bv, gv = _elems(beta, 1), _elems(gamma, 1)
    sd, pf = (np.frombuffer(bytes(x), dtype=np.uint8) for x in (seed, proof))
    if sd.shape[0] != 32 or pf.shape[0] == 0 or not 1 <= k <= 16:
        raise _bad_arg()
    point, claims, ok = np.zeros((max(n_vars, 1), 4), dtype=np.uint64), np.zeros((2 * k, 4), dtype=np.uint64), c.c_int32()
    check(lib.zk_perm_verify_host(field, n_vars, k, _p(bv), _p(gv), sd.ctypes.data_as(u8p), pf.ctypes.data_as(u8p), pf.shape[0], _p(point),
                                  _p(claims), c.byref(ok)))
    return (point, claims) if ok.value else None


def bench_perm(w, sigma, path=0, reps=5):
    """device ms (zk_bench_perm): path 0 the fingerprint table and its product tree on the default route, 1 on the unfused route, 3 on the
    fused route, 2 the whole proof"""
    w, sigma = list(w), list(sigma)
    if not w or len(w) != len(sigma):
        raise _bad_arg()
    ms = c.c_double()
    wp, _k1 = _handles(w)
    sp, _k2 = _handles(sigma)
    check(lib.zk_bench_perm(w[0].ctx._h, wp, sp, len(w), path, reps, c.byref(ms)))
    return ms.value


# ---- fractional-sum (LogUp) argument and lookups (zk_mle_fraction_tree, zk_fsum_*, zk_lookup_multiplicities; tests/fsum_ref.py is the definition)
def fsum_proof_bytes(n_vars):
    n = c.c_uint64()
    check(lib.zk_fsum_proof_bytes(n_vars, c.byref(n)))
    return n.value


def fraction_tree(q, p=None, shift=None):
    """(heap_p, heap_q): the fraction tree over p / (q + shift) as two new tables in heap order (zk_mle_fraction_tree): out[2^j + i] =
    level j, so heap_p[1] / heap_q[1] = sum_i p[i] / (q[i] + shift); p None = all ones.  Stream-ordered, no host wait."""
    sv = _shift_arg(shift)
    hp, hq = c.c_void_p(), c.c_void_p()
    check(lib.zk_mle_fraction_tree(q.ctx._h, None if p is None else p._h, q._h, None if sv is None else _p(sv), c.byref(hp), c.byref(hq)))
    return MultiLinearPolynomial(q.ctx, hp), MultiLinearPolynomial(q.ctx, hq)


def fractional_sum_prove(q, seed, p=None, shift=None):
    """(total, proof, point, claims) of zk_fsum_prove: total = (N, D) with N / D = sum_i p[i] / (q[i] + shift) as (2, 4) limbs, the proof
    bytes, and the claims p(point) = claims[0], q(point) = claims[1] the verifier will be left with (point: (n_vars, 4) limbs).  p None =
    all ones.  The seed must bind the tables (their commitments' roots)."""
    sv = _shift_arg(shift)
    sd = np.frombuffer(bytes(seed), dtype=np.uint8)
    if sd.shape[0] != 32:
        raise _bad_arg()
    n = q.n_vars()
    total, claims = np.zeros((2, 4), dtype=np.uint64), np.zeros((2, 4), dtype=np.uint64)
    point = np.zeros((max(n, 1), 4), dtype=np.uint64)
    proof = np.zeros(fsum_proof_bytes(n), dtype=np.uint8)
    check(lib.zk_fsum_prove(q.ctx._h, None if p is None else p._h, q._h, None if sv is None else _p(sv), sd.ctypes.data_as(u8p), _p(total),
                            proof.ctypes.data_as(u8p), _p(point), _p(claims)))
    return total, proof.tobytes(), point, claims


def fractional_sum_verify(field, n_vars, has_p, seed, total, proof, shift=None):
    """host only (zk_fsum_verify_host): (point, claims) -- what is left to check is p(point) == claims[0] (already checked to be 1 when
    has_p is false) and q(point) == claims[1] -- or None when the proof is rejected (D = 0 included)"""
    sv, tv = _shift_arg(shift), _elems(total, 2)
    sd, pf = (np.frombuffer(bytes(x), dtype=np.uint8) for x in (seed, proof))
    if sd.shape[0] != 32 or pf.shape[0] == 0:
        raise _bad_arg()
    point, claims, ok = np.zeros((max(n_vars, 1), 4), dtype=np.uint64), np.zeros((2, 4), dtype=np.uint64), c.c_int32()
    check(lib.zk_fsum_verify_host(field, n_vars, 1 if has_p else 0, None if sv is None else _p(sv), sd.ctypes.data_as(u8p), _p(tv),
                                  pf.ctypes.data_as(u8p), pf.shape[0], _p(point), _p(claims), c.byref(ok)))
    return (point, claims) if ok.value else None


def lookup_multiplicities(table, witness):
    """(m, missing, first_missing, duplicates) of zk_lookup_multiplicities: m[j] = #{i : witness[i] = table[j]} as a new table if j is the
    lowest index holding that value, else 0; missing = the witness entries found nowhere in the table, first_missing the lowest such index
    (2^64 - 1: none); duplicates = len(table) - #distinct values"""
    h = c.c_void_p()
    missing, first, dup = c.c_uint64(), c.c_uint64(), c.c_uint64()
    check(lib.zk_lookup_multiplicities(table.ctx._h, table._h, witness._h, c.byref(h), c.byref(missing), c.byref(first), c.byref(dup)))
    return MultiLinearPolynomial(table.ctx, h), missing.value, first.value, dup.value


def _lookup_seeds(seed):
    if len(bytes(seed)) != 32:
        raise _bad_arg()
    return keccak256(bytes(seed) + b"\x00"), keccak256(bytes(seed) + b"\x01")


def lookup_prove(witness, table, alpha, seed):
    """(m, proof): every entry of `witness` occurs in `table` (tests/fsum_ref.py lookup_prove), made of lookup_multiplicities and two
    fractional_sum_prove calls only: sum_i 1 / (witness[i] + alpha) on keccak256(seed | 0) and sum_j m[j] / (table[j] + alpha) on
    keccak256(seed | 1); proof = (total_f, proof_f, total_t, proof_t).  Raises ValueError naming first_missing when a witness entry is
    absent from the table.  m must be committed, and bound by `seed` together with witness and table, BEFORE alpha is drawn; the argument
    is sound only when the witness has fewer entries than the field's characteristic."""
    m, missing, first_missing, _ = lookup_multiplicities(table, witness)
    if missing:
        m.free()
        raise ValueError(f"witness entry {first_missing} (first_missing) is not in the table; {missing} entries are missing")
    sf, st = _lookup_seeds(seed)
    total_f, proof_f, _, _ = fractional_sum_prove(witness, sf, None, alpha)
    total_t, proof_t, _, _ = fractional_sum_prove(table, st, m, alpha)
    return m, (total_f, proof_f, total_t, proof_t)


def lookup_verify(field, n_witness, n_table, alpha, seed, proof):
    """host only: None, or ((r_f, f_claim), (r_t, t_claim, m_claim)) -- what is left to check is witness(r_f) == f_claim, table(r_t) ==
    t_claim and m(r_t) == m_claim, e.g. by mlpcs_verify against the three commitments.  Accepted iff both fractional sums verify and
    N_f D_t == N_t D_f.  See lookup_prove for what the seed must bind and for the bound on the witness's size."""
    total_f, proof_f, total_t, proof_t = proof
    sf, st = _lookup_seeds(seed)
    got_f = fractional_sum_verify(field, n_witness, False, sf, total_f, proof_f, alpha)
    got_t = fractional_sum_verify(field, n_table, True, st, total_t, proof_t, alpha)
    if got_f is None or got_t is None:
        return None
    (nf, df), (nt, dt) = fe_to_ints(field, total_f), fe_to_ints(field, total_t)
    if (nf * dt - nt * df) % modulus(field):
        return None
    return (got_f[0], got_f[1][1]), (got_t[0], got_t[1][1], got_t[1][0])


def bench_fsum(q, path=0, reps=5):
    """device ms (zk_bench_fsum): path 0 the fraction tree on the default route (p = ones), 1 one level per launch, 2 the whole proof,
    3 lookup_multiplicities' launches with the witness equal to the table"""
    ms = c.c_double()
    check(lib.zk_bench_fsum(q.ctx._h, q._h, path, reps, c.byref(ms)))
    return ms.value


def upoly_inverse_series_host(ctx, f, k):
    """value-semantics series inverse (zk_upoly_inverse_series_host): the k coefficients of 1 / f mod z^k"""
    fv = _elems(f)
    out = np.zeros((max(k, 1), 4), dtype=np.uint64)
    check(lib.zk_upoly_inverse_series_host(ctx._h, _p(fv), fv.shape[0], k, _p(out)))
    return out[:k]


class CoeffMultilinearPolynomial:
    """polynomial::multilinear::coefficient_form::CoeffMultilinearPolynomial (coefficient_form.rs:27-30), only as the
    producer of evaluation tables: ::new (:158-176), ::new_with_coefficient (:178-193), ::to_evaluation_form (:340-347,
    computed on the GPU and left resident as a MultiLinearPolynomial)."""

    def __init__(self, field, n_vars, coefficients):
        # {key: element}, key bit v <-> variable v.  The term map is IMMUTABLE (the reference's BTreeMap is a private field,
        # coefficient_form.rs:27-30): a private copy, exposed read-only, flattened once into the two arrays the library takes
        import types

        self.field, self._n_vars = field, n_vars
        self._terms = {int(k): np.array(v, dtype=np.uint64).reshape(4) for k, v in dict(coefficients).items()}
        self.coefficients = types.MappingProxyType(self._terms)
        keys = np.array(sorted(self._terms), dtype=np.uint64)
        coeffs = np.stack([self._terms[int(k)] for k in keys]) if len(keys) else np.zeros((0, 4), dtype=np.uint64)
        for v in self._terms.values():
            v.setflags(write=False)
        self._flat = (keys, np.ascontiguousarray(coeffs, dtype=np.uint64))

    @classmethod
    def new(cls, field, number_of_variables, terms):
        """terms: [(coefficient element, [bool] * n_vars)]; duplicate selectors are summed (:164-171)."""
        p = modulus(field)
        acc = {}
        for coeff, selector in terms:
            if len(selector) != number_of_variables:
                raise ZkError(-20, "the selector array len should be the same as the number of variables")
            key = sum(1 << v for v, present in enumerate(selector) if present)          # selector_to_index :418-430
            acc[key] = (acc.get(key, 0) + fe_to_int(field, coeff)) % p
        return cls(field, number_of_variables, {k: fe_from_int(field, v) for k, v in acc.items()})

    @classmethod
    def new_with_coefficient(cls, field, number_of_variables, coefficients):
        if coefficients and max(coefficients) >= (1 << number_of_variables):
            raise ZkError(-10, "coefficient map represents more than specificed number of variables")
        return cls(field, number_of_variables, dict(coefficients))

    def n_vars(self):
        return self._n_vars

    def to_evaluation_form(self, ctx):
        keys, coeffs = self._flat
        h = c.c_void_p()
        check(lib.zk_coeff_to_evaluation(ctx._h, self._n_vars, _p(keys), _p(coeffs), len(keys), c.byref(h)))
        return MultiLinearPolynomial(ctx, h)

    # CoeffMultilinearPolynomial::interpolate (coefficient_form.rs:200-216), computed on the GPU
    @classmethod
    def interpolate(cls, ctx, values):
        """every key 0 .. 2^n - 1 present (zeros included), n = bit length of len - 1 (1 for a single value); no value: n = 0, no key"""
        if isinstance(values, MultiLinearPolynomial):
            return DeviceCoeffMultilinear.interpolate(ctx, values).to_host()
        n, dense = cmle_interpolate_host(ctx, values)
        return cls(ctx.field, n, dict(enumerate(dense)))


def _cmle_n_vars_for_len(length):   # bit_count_for_n_elem (coefficient_form.rs:517-523): len(format!("{:b}", len - 1))
    return max(1, (length - 1).bit_length())


def cmle_interpolate_host(ctx, values):
    """value-semantics interpolate (zk_cmle_interpolate_host): (n_vars, the 2^n_vars coefficients in key order); no value: (0, empty)"""
    v = _elems(values)
    n = _cmle_n_vars_for_len(v.shape[0]) if v.shape[0] else 0
    out = np.zeros((1 << n if v.shape[0] else 1, 4), dtype=np.uint64)
    nv = c.c_uint64()
    check(lib.zk_cmle_interpolate_host(ctx._h, _p(v), v.shape[0], c.byref(nv), _p(out)))
    return nv.value, out[:(1 << nv.value) if v.shape[0] else 0]


class DeviceCoeffMultilinear:
    """A CoeffMultilinearPolynomial resident in HBM (zk_cmle): the coefficients of its present keys in key order (key bit v <-> variable
    v).  upload and interpolate make one with every key 0 .. 2^n_vars - 1 present.  partial_evaluate removes exactly the keys that have
    a bit of a fixed variable, so the present keys are always {k : k & fixed_mask() == 0}; the object holds their 2^(n_vars -
    popcount(fixed_mask())) coefficients, ascending, and coefficients(), to_bytes(), to_host() and evaluate_slice() speak of those keys
    only, as the reference's BTreeMap does.  relabel() renames the variables that are left (no data moves); scalar_multiply works on any
    such object; + and * need every key present (relabel first), and to_evaluation_form() does too (ZkError -25 otherwise).

    One divergence, in * only: the reference's Mul skips every pair with a zero coefficient (coefficient_form.rs:393-395), so the keys
    only such pairs reach are absent from its product; here they are present with coefficient zero.  Equal as polynomials; key for key
    and byte for byte equal when no operand coefficient is zero."""

    def __init__(self, ctx, handle):
        self.ctx, self._h = ctx, handle

    @classmethod
    def upload(cls, ctx, n_vars, dense):
        co = _elems(dense)
        h = c.c_void_p()
        check(lib.zk_cmle_upload(ctx._h, n_vars, _p(co), co.shape[0], c.byref(h)))
        return cls(ctx, h)

    # ::interpolate (coefficient_form.rs:200-216): from a resident table (one value gives n_vars 1) or from an array of any length >= 1
    @classmethod
    def interpolate(cls, ctx, values):
        if isinstance(values, MultiLinearPolynomial):
            h = c.c_void_p()
            check(lib.zk_cmle_interpolate(ctx._h, values._h, c.byref(h)))
            return cls(ctx, h)
        v = _elems(values)
        if v.shape[0] and v.shape[0] & (v.shape[0] - 1) == 0:
            return cls.interpolate(ctx, MultiLinearPolynomial.new(ctx, v.shape[0].bit_length() - 1, v))
        if not v.shape[0]:
            raise ValueError("DeviceCoeffMultilinear.interpolate: no values (the reference's empty map has no dense form)")
        n, dense = cmle_interpolate_host(ctx, v)
        return cls.upload(ctx, n, dense)

    def free(self):
        if getattr(self, "_h", None) and getattr(self.ctx, "_h", None):
            lib.zk_cmle_free(self.ctx._h, self._h)
        self._h = None

    def __del__(self):
        self.free()

    def n_vars(self):
        n = c.c_uint64()
        check(lib.zk_cmle_n_vars(self._h, c.byref(n)))
        return n.value

    def fixed_mask(self):
        """bit v set <-> variable v has been fixed by partial_evaluate: no present key has bit v"""
        m = c.c_uint64()
        check(lib.zk_cmle_fixed_mask(self._h, c.byref(m)))
        return m.value

    def __len__(self):
        """number of present keys: 2^(n_vars - popcount(fixed_mask))"""
        n = c.c_uint64()
        check(lib.zk_cmle_len(self._h, c.byref(n)))
        return n.value

    def keys(self):
        """the present keys, ascending: pdep(j, ~fixed_mask) for j = 0 .. len - 1"""
        j = np.arange(len(self), dtype=np.uint64)
        fixed, keys, at = self.fixed_mask(), np.zeros(len(self), dtype=np.uint64), 0
        for v in range(self.n_vars()):
            if not fixed >> v & 1:
                keys |= ((j >> np.uint64(at)) & np.uint64(1)) << np.uint64(v)
                at += 1
        return keys

    def coefficients(self):
        """the coefficients of the present keys, ascending key order: (len, 4); index = key while fixed_mask() == 0"""
        out = np.zeros((len(self), 4), dtype=np.uint64)
        check(lib.zk_cmle_download(self.ctx._h, self._h, _p(out)))
        return out

    def to_host(self):
        return CoeffMultilinearPolynomial(self.ctx.field, self.n_vars(), dict(zip((int(k) for k in self.keys()), self.coefficients())))

    # partial_evaluate (coefficient_form.rs:72-104): [(selector, element)], selector a bool sequence with exactly one True.  A selector
    # longer than n_vars is skipped, a shorter one is ZkError(-13), zero or several True ZkError(-14); the first assignment of a variable
    # wins.  A new object; this one is unchanged.
    def partial_evaluate(self, assignments):
        assignments = list(assignments)
        lens = np.array([len(sel) for sel, _ in assignments], dtype=np.uint64)
        flat = np.array([1 if b else 0 for sel, _ in assignments for b in sel], dtype=np.uint8)
        vals = np.ascontiguousarray([np.asarray(v, dtype=np.uint64).reshape(4) for _, v in assignments], dtype=np.uint64).reshape(-1, 4)
        pad8, pad64 = np.zeros(1, dtype=np.uint8), np.zeros((1, 4), dtype=np.uint64)
        h = c.c_void_p()
        check(lib.zk_cmle_partial_evaluate(self.ctx._h, self._h, (flat if flat.size else pad8).ctypes.data_as(u8p), _p(lens if lens.size else pad64),
                                           _p(vals if vals.size else pad64), len(assignments), c.byref(h)))
        return DeviceCoeffMultilinear(self.ctx, h)

    # relabel (coefficient_form.rs:109-123), in place (the reference consumes self): returns self
    def relabel(self):
        check(lib.zk_cmle_relabel(self.ctx._h, self._h))
        return self

    # scalar_multiply (coefficient_form.rs:272-282)
    def scalar_multiply(self, s):
        h = c.c_void_p()
        check(lib.zk_cmle_scalar_multiply(self.ctx._h, self._h, _p(np.ascontiguousarray(s, dtype=np.uint64).reshape(4)), c.byref(h)))
        return DeviceCoeffMultilinear(self.ctx, h)

    # Add (coefficient_form.rs:350-373): n_vars of the operand with more keys, of `other` on a tie
    def __add__(self, other):
        if not isinstance(other, DeviceCoeffMultilinear):
            return NotImplemented
        h = c.c_void_p()
        check(lib.zk_cmle_add(self.ctx._h, self._h, other._h, c.byref(h)))
        return DeviceCoeffMultilinear(self.ctx, h)

    # Mul (coefficient_form.rs:375-415): this object's variables first; zero coefficients are kept (class docstring)
    def __mul__(self, other):
        if not isinstance(other, DeviceCoeffMultilinear):
            return NotImplemented
        h = c.c_void_p()
        check(lib.zk_cmle_mul(self.ctx._h, self._h, other._h, c.byref(h)))
        return DeviceCoeffMultilinear(self.ctx, h)

    # evaluate_slice (coefficient_form.rs:39-69): fewer assignments than variables -> ZkError(-12); extra ones are ignored
    def evaluate_slice(self, point):
        pt = np.ascontiguousarray(point, dtype=np.uint64).reshape(-1, 4)
        out = np.zeros(4, dtype=np.uint64)
        check(lib.zk_cmle_evaluate(self.ctx._h, self._h, _p(pt if pt.size else np.zeros((1, 4), dtype=np.uint64)), pt.shape[0], _p(out)))
        return out

    # to_evaluation_form (coefficient_form.rs:340-347), left resident
    def to_evaluation_form(self):
        h = c.c_void_p()
        check(lib.zk_cmle_to_evaluation(self.ctx._h, self._h, c.byref(h)))
        return MultiLinearPolynomial(self.ctx, h)

    # to_bytes (coefficient_form.rs:131-139): 4 + 40 * len bytes
    def to_bytes_array(self):
        out = np.empty(4 + 40 * len(self), dtype=np.uint8)
        check(lib.zk_cmle_to_bytes(self.ctx._h, self._h, out.ctypes.data_as(u8p)))
        return out

    def to_bytes(self):
        return self.to_bytes_array().tobytes()

    def bench(self, op, table=None, point=None, reps=10):
        """average device ms of interpolate (op 0, of `table`), to_evaluation (op 1) or evaluate (op 2, at `point`) (zk_bench_cmle)"""
        pt = np.ascontiguousarray(point if point is not None else np.zeros((0, 4)), dtype=np.uint64).reshape(-1, 4)
        out = c.c_double()
        check(lib.zk_bench_cmle(self.ctx._h, op, table._h if table is not None else None, self._h, _p(pt if pt.size else np.zeros((1, 4), dtype=np.uint64)),
                                pt.shape[0], reps, c.byref(out)))
        return out.value

    def bench_algebra(self, op, other=None, assignments=(), scalar=None, reps=10):
        """average device ms of partial_evaluate(assignments) (op 0), + other (1),
        scalar_multiply(scalar) (2) or * other (3) (zk_bench_cmle_algebra)"""
        assignments = list(assignments)
        lens = np.array([len(sel) for sel, _ in assignments] or [0], dtype=np.uint64)
        flat = np.array([1 if b else 0 for sel, _ in assignments for b in sel] or [0], dtype=np.uint8)
        vals = [np.asarray(v, dtype=np.uint64).reshape(4) for _, v in assignments] if op != 2 else [np.asarray(scalar, dtype=np.uint64).reshape(4)]
        vals = np.ascontiguousarray(vals or [np.zeros(4, dtype=np.uint64)], dtype=np.uint64)
        out = c.c_double()
        check(lib.zk_bench_cmle_algebra(self.ctx._h, op, self._h, other._h if other is not None else None, flat.ctypes.data_as(u8p), _p(lens),
                                        _p(vals), len(assignments), reps, c.byref(out)))
        return out.value


class ProductPoly:
    """P(x) = A(x).B(x).C(x) (product_poly.rs:7-10)."""

    def __init__(self, polynomials):
        self.polynomials = list(polynomials)
        self.ctx = self.polynomials[0].ctx

    # ProductPoly::new (product_poly.rs:14-32)
    @classmethod
    def new(cls, polynomials):
        polynomials = list(polynomials)
        hp, keep = _handles(polynomials)
        check(lib.zk_product_check(hp, len(polynomials)))
        return cls(polynomials)

    def n_vars(self):  # product_poly.rs:86
        return self.polynomials[0].n_vars()

    def evaluate(self, assignments):  # product_poly.rs:36-44
        a = _elems(assignments)
        hp, keep = _handles(self.polynomials)
        out = np.zeros(4, dtype=np.uint64)
        check(lib.zk_product_evaluate(self.ctx._h, hp, len(self.polynomials), _p(a), a.shape[0], _p(out)))
        return out

    def partial_evaluate(self, initial_var, assignments):  # product_poly.rs:48-63
        return ProductPoly([q.partial_evaluate(initial_var, assignments) for q in self.polynomials])

    def prod_reduce_device(self):
        """prod_reduce with the result left resident: a new MultiLinearPolynomial (the reference returns a Vec<F>)"""
        hp, keep = _handles(self.polynomials)
        h = c.c_void_p()
        check(lib.zk_prod_reduce(self.ctx._h, hp, len(self.polynomials), c.byref(h)))
        return MultiLinearPolynomial(self.ctx, h)

    def prod_reduce(self):  # product_poly.rs:66-74
        return self.prod_reduce_device().evaluation_slice()

    def round_sums(self, max_var_degree):  # prover.rs:49-56 for one round
        hp, keep = _handles(self.polynomials)
        out = np.zeros((max_var_degree + 1, 4), dtype=np.uint64)
        check(lib.zk_round_sums(self.ctx._h, hp, len(self.polynomials), max_var_degree, _p(out)))
        return out

    def to_bytes(self):  # product_poly.rs:77-83
        return b"".join(q.to_bytes() for q in self.polynomials)

    def clone(self):
        return ProductPoly([q.clone() for q in self.polynomials])


class SumcheckProof:
    """sumcheck::SumcheckProof (sumcheck/src/lib.rs:8-11)."""

    def __init__(self, sum_, round_polys):
        self.sum, self.round_polys = sum_, round_polys


class SubClaim:
    """sumcheck::SubClaim (sumcheck/src/lib.rs:17-20)."""

    def __init__(self, sum_, challenges):
        self.sum, self.challenges = sum_, challenges


class SumcheckProver:
    """SumcheckProver::<MAX_VAR_DEGREE, F> (prover.rs:9-73); MAX_VAR_DEGREE is the constructor argument."""

    def __init__(self, max_var_degree):
        self.max_var_degree = max_var_degree

    def _run(self, poly, sum_, absorb, consume):
        D, n, k = self.max_var_degree, poly.n_vars(), len(poly.polynomials)
        s = _elems(sum_, 1)
        rp = np.zeros((n, D + 1, 4), dtype=np.uint64)
        ch = np.zeros((n, 4), dtype=np.uint64)
        hp, keep = _handles(poly.polynomials)
        check(lib.zk_sumcheck_prove(poly.ctx._h, hp, k, D, _p(s), int(absorb), int(consume), _p(rp), _p(ch)))
        return SumcheckProof(s.reshape(4).copy(), rp), ch

    def prove_partial_batch(self, polys, sums, consume=False):
        """len(polys) independent prove_partial calls (prover.rs:24-30), one ProductPoly each, same number of factors and variables,
        proved side by side (zk_sumcheck_prove_batch: one launch per round for all proofs).  Returns [(SumcheckProof, challenges)], each
        pair equal to what prove_partial(poly, sum) returns."""
        polys = list(polys)
        if not polys:
            return []
        D, n, k = self.max_var_degree, polys[0].n_vars(), len(polys[0].polynomials)
        if any(len(q.polynomials) != k for q in polys):
            raise ValueError("prove_partial_batch: every ProductPoly must have the same number of factors")
        B = len(polys)
        s = _elems(sums, B)
        rp = np.zeros((B, n, D + 1, 4), dtype=np.uint64)
        ch = np.zeros((B, n, 4), dtype=np.uint64)
        hp, keep = _handles([f for q in polys for f in q.polynomials])
        check(lib.zk_sumcheck_prove_batch(polys[0].ctx._h, B, hp, k, D, _p(s), int(consume), _p(rp), _p(ch)))
        return [(SumcheckProof(s[b].copy(), rp[b]), ch[b]) for b in range(B)]

    def prove(self, poly, sum_, consume=False):  # prover.rs:15-20
        return self._run(poly, sum_, True, consume)[0]

    def prove_partial(self, poly, sum_, consume=False):  # prover.rs:24-30
        return self._run(poly, sum_, False, consume)


def _ragged_rounds(round_polys):
    """SumcheckProof.round_polys is a Vec<Vec<F>> (sumcheck/src/lib.rs:8-11): a (rounds, D+1, 4) array, or a list of
    per-round (len_r, 4) arrays of different lengths -> (lens uint32, the evaluations back to back)."""
    if isinstance(round_polys, np.ndarray) and round_polys.ndim == 3:
        rp = np.ascontiguousarray(round_polys, dtype=np.uint64)
        lens = np.full(rp.shape[0] + 1, rp.shape[1], dtype=np.uint32)
        return rp.shape[0], lens, rp.reshape(-1, 4) if rp.size else np.zeros((1, 4), dtype=np.uint64)
    rounds = [np.ascontiguousarray(r, dtype=np.uint64).reshape(-1, 4) for r in round_polys]
    lens = np.array([r.shape[0] for r in rounds] + [0], dtype=np.uint32)
    flat = np.concatenate(rounds + [np.zeros((1, 4), dtype=np.uint64)], axis=0)
    return len(rounds), lens, np.ascontiguousarray(flat)


class SumcheckVerifier:
    """SumcheckVerifier::<F> (verifier.rs:9-78).  Each round polynomial is interpolated at its own length, as
    verifier.rs:55-58 does (round_polys may be a list of arrays of different lengths)."""

    @staticmethod
    def verify(poly, proof):  # verifier.rs:15-33
        n_rp, lens, rp = _ragged_rounds(proof.round_polys)
        hp, keep = _handles(poly.polynomials)
        ok = c.c_int32()
        s = _elems(proof.sum, 1)
        check(lib.zk_sumcheck_verify_lengths(poly.ctx._h, hp, len(poly.polynomials), n_rp,
                                             lens.ctypes.data_as(c.POINTER(c.c_uint32)), _p(s), _p(rp), c.byref(ok)))
        return bool(ok.value)

    @staticmethod
    def verify_partial(field, proof):  # verifier.rs:38-41
        n_rp, lens, rp = _ragged_rounds(proof.round_polys)
        s = _elems(proof.sum, 1)
        sub = np.zeros(4, dtype=np.uint64)
        ch = np.zeros((max(n_rp, 1), 4), dtype=np.uint64)
        check(lib.zk_sumcheck_verify_partial_lengths(field, n_rp, lens.ctypes.data_as(c.POINTER(c.c_uint32)), _p(s), _p(rp),
                                                     _p(sub), _p(ch)))
        return SubClaim(sub, ch[:n_rp])


# ---- fft crate (fft/src/lib.rs) ---------------------------------------------------------------------------------
def _fft_call(fn, ctx, values, *extra):
    v = _elems(values)
    out = np.zeros_like(v)
    check(fn(ctx._h, _p(v), v.shape[0], *extra, _p(out)))
    return out


def fft(ctx, coefficients):  # fft/src/lib.rs:4-8
    return _fft_call(lib.zk_fft_host, ctx, coefficients)


def ifft(ctx, evaluations):  # fft/src/lib.rs:11-19
    return _fft_call(lib.zk_ifft_host, ctx, evaluations)


def fft_internal(ctx, values, omega):  # fft/src/lib.rs:21-46
    w = _elems(omega, 1)
    return _fft_call(lib.zk_fft_internal_host, ctx, values, _p(w))


def ntt(ctx, vec_in, vec_out, inverse=False):
    """device-resident form: MultiLinearPolynomial handles double as vectors of 2^n elements."""
    check(lib.zk_ntt(ctx._h, vec_in._h, int(inverse), vec_out._h))
    return vec_out


def batch_last_stats():
    """(launches merged for all proofs, launches replayed proof by proof) of this thread's last prove_partial_batch"""
    a, b = c.c_uint64(), c.c_uint64()
    check(lib.zk_batch_last_stats(c.byref(a), c.byref(b)))
    return a.value, b.value


def bench_prove_partial(poly, max_var_degree, sum_, reps=10):
    """per-call wall clock (ms) of `reps` prove_partial calls measured inside the library with std::chrono (what a compiled host
    sees: no binding overhead)"""
    hp, keep = _handles(poly.polynomials)
    out = (c.c_double * reps)()
    check(lib.zk_bench_prove_partial(poly.ctx._h, hp, len(poly.polynomials), int(max_var_degree), _p(np.ascontiguousarray(sum_, dtype=np.uint64)),
                                     reps, out))
    return [float(v) for v in out]


def bench_evaluate(table, point, reps=10):
    """per-call wall clock (ms) of `reps` evaluate calls measured inside the library with std::chrono"""
    pt = np.ascontiguousarray(point, dtype=np.uint64).reshape(-1, 4)
    out = (c.c_double * reps)()
    check(lib.zk_bench_evaluate(table.ctx._h, table._h, _p(pt if pt.size else np.zeros((1, 4), dtype=np.uint64)), pt.shape[0], reps, out))
    return [float(v) for v in out]


def bench_evaluate_device(table, point, reps=20):
    """average device time (ms) of one evaluate: `reps` back-to-back enqueues between two HIP events, no host wait in between"""
    pt = np.ascontiguousarray(point, dtype=np.uint64).reshape(-1, 4)
    out = c.c_double()
    check(lib.zk_bench_evaluate_device(table.ctx._h, table._h, _p(pt if pt.size else np.zeros((1, 4), dtype=np.uint64)), pt.shape[0], reps, c.byref(out)))
    return out.value


def bench_ntt(ctx, vec_in, vec_out, inverse=False, reps=5):
    ms = c.c_double()
    check(lib.zk_bench_ntt(ctx._h, vec_in._h, int(inverse), vec_out._h, reps, c.byref(ms)))
    return ms.value


__all__ = [
    "BN254_FR", "BLS12_381_FR", "BLS12_377_FR", "Context", "MultiLinearPolynomial", "UnivariatePolynomial", "upoly_mul_host", "upoly_interpolate_host", "upoly_evaluate_many_host", "upoly_divrem_host", "upoly_inverse_series_host", "batch_inverse_host", "MerkleTree", "merkle_verify", "fri_lde", "fri_fold", "fri_prove", "fri_verify", "fri_proof_bytes", "bench_fri_fold", "PolyCommitment", "pcs_verify", "pcs_proof_bytes", "deep_quotient", "bench_deep_quotient", "MultilinearCommitment", "mlpcs_verify", "mlpcs_proof_bytes", "eq_sums", "bench_mlpcs_round", "MultilinearBatchCommitment", "mlbatch_verify", "mlbatch_proof_bytes", "lincomb", "eq_sums_many", "bench_mlbatch", "product_tree", "grand_product_prove", "grand_product_verify", "grand_product_verify_table", "gprod_proof_bytes", "bench_gprod", "fraction_tree", "fractional_sum_prove", "fractional_sum_verify", "fsum_proof_bytes", "lookup_multiplicities", "lookup_prove", "lookup_verify", "bench_fsum", "Gate", "zerocheck_prove", "zerocheck_verify", "zerocheck_proof_bytes", "gate_sums", "bench_zerocheck", "perm_fingerprint", "permutation_prove", "permutation_verify", "perm_proof_bytes", "bench_perm", "wiring_sigma","CoeffMultilinearPolynomial", "DeviceCoeffMultilinear", "cmle_interpolate_host", "ProductPoly", "SumcheckProof",
    "SubClaim", "SumcheckProver", "SumcheckVerifier", "Transcript", "ZkError", "fft", "ifft", "fft_internal", "ntt", "bench_ntt", "bench_prove_partial", "batch_last_stats", "bench_evaluate", "bench_evaluate_device",
    "fe_from_int", "fe_from_ints", "fe_to_int", "fe_to_ints", "keccak256", "modulus", "two_adicity", "root_of_unity", "mask", "index_pair",
]
