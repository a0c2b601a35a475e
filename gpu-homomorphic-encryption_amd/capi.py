"""ctypes binding of include/fhe_hip.h.  Thin by design: every call goes straight to the C ABI and
raises FheError on a non-zero status (no CPU fallback anywhere)."""
import ctypes
import os

import numpy as np

from .build import library_path

WIDTH_32, WIDTH_64, WIDTH_52, WIDTH_256, WIDTH_64X = 1, 2, 3, 4, 5
_lib = None

U64x4 = ctypes.c_uint64 * 4


class FheError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"fhe_hip error {code}: {msg}")
        self.code = code


def lib():
    """Load libfhe_hip.so.  Fails loudly if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise FheError(-100, f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                             "(there is no CPU fallback for the HIP engine)")
    L = ctypes.CDLL(path)
    vp, u32, u64, sz, ci = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_int
    P = ctypes.POINTER
    sigs = {
        "fhe_hip_abi_version": ([], ci),
        "fhe_hip_last_error": ([], ctypes.c_char_p),
        "fhe_hip_device_count": ([P(ci)], ci),
        "fhe_hip_set_device": ([ci], ci),
        "fhe_hip_get_device": ([P(ci)], ci),
        "fhe_hip_device_name": ([ctypes.c_char_p, sz], ci),
        "fhe_hip_malloc": ([P(vp), sz], ci),
        "fhe_hip_free": ([vp], ci),
        "fhe_hip_memset": ([vp, ci, sz], ci),
        "fhe_hip_memcpy_h2d": ([vp, vp, sz], ci),
        "fhe_hip_memcpy_d2h": ([vp, vp, sz], ci),
        "fhe_hip_memcpy_d2d": ([vp, vp, sz], ci),
        "fhe_hip_sync": ([], ci),
        "fhe_montgomery_inverse": ([U64x4, U64x4], ci),
        "fhe_montgomery_params": ([U64x4, U64x4, U64x4], ci),
        "fhe_find_ntt_primes": ([u32, u32, u32, P(u64)], ci),
        "fhe_find_ntt_primes_wide": ([u32, u32, u32, vp], ci),
        "fhe_find_psi": ([u32, U64x4, U64x4], ci),
        "fhe_u256_add_mod": ([vp, vp, vp, U64x4, sz, vp], ci),
        "fhe_u256_sub_mod": ([vp, vp, vp, U64x4, sz, vp], ci),
        "fhe_u256_mont_mul": ([vp, vp, vp, U64x4, u64, sz, vp], ci),
        "fhe_u256_mont_mul_scalar": ([vp, vp, U64x4, U64x4, u64, sz, vp], ci),
        "fhe_ntt_create": ([P(vp), u32, U64x4], ci),
        "fhe_ntt_destroy": ([vp], ci),
        "fhe_ntt_set_stream": ([vp, vp], ci),
        "fhe_ntt_width_class": ([vp], ci),
        "fhe_ntt_forward": ([vp, vp, u32], ci),
        "fhe_ntt_inverse": ([vp, vp, u32], ci),
        "fhe_ntt_pointwise": ([vp, vp, vp, vp, u32], ci),
        "fhe_ntt_multiply": ([vp, vp, vp, vp, u32], ci),
        "fhe_rns_ntt_create": ([P(vp), u32, vp, u32], ci),
        "fhe_rns_ntt_destroy": ([vp], ci),
        "fhe_rns_ntt_set_stream": ([vp, vp], ci),
        "fhe_rns_ntt_width_class": ([vp], ci),
        "fhe_rns_ntt_reserve": ([vp, u32], ci),
        "fhe_rns_ntt_workspace_bytes": ([vp, ctypes.POINTER(ctypes.c_uint64)], ci),
        "fhe_rns_ntt_forward": ([vp, vp, u32], ci),
        "fhe_rns_ntt_inverse": ([vp, vp, u32], ci),
        "fhe_rns_ntt_pointwise": ([vp, vp, vp, vp, u32], ci),
        "fhe_rns_ntt_multiply": ([vp, vp, vp, vp, u32], ci),
        "fhe_rns_poly_add": ([vp, vp, vp, vp, u32], ci),
        "fhe_rns_poly_sub": ([vp, vp, vp, vp, u32], ci),
        "fhe_ct_multiply": ([vp] * 8 + [u32], ci),
        "fhe_rns_check_canonical": ([vp, vp, u32], ci),
        "fhe_rns_to_rns": ([vp, vp, vp, u32], ci),
        "fhe_rns_from_rns": ([vp, vp, vp, u32], ci),
        "fhe_rns_monomial_mul_sub": ([vp, vp, vp, vp, u32], ci),
        "fhe_blind_rotate_step": ([vp, vp, vp, vp, vp, vp, vp, vp, u32], ci),
        "fhe_blind_rotate": ([vp, P(vp), P(vp), u32, vp, vp, vp, vp, vp, u32], ci),
        "fhe_rns_fast_base_convert": ([vp, vp, vp, vp, u32], ci),
        "fhe_rns_base_create": ([P(vp), vp, u32], ci),
        "fhe_rns_ntt_multiply_bcast": ([vp, vp, vp, vp, u32], ci),
        "fhe_rns_mul_mont_literal": ([vp, vp, vp, vp, u32], ci),
        "fhe_ref_forward_kernel_literal": ([vp, vp, U64x4, u64, u32, u32, vp], ci),
        "fhe_ref_inverse_kernel_literal": ([vp, vp, U64x4, u64, U64x4, u32, u32, vp], ci),
        "fhe_ref_stockham_stage_literal": ([vp, vp, vp, U64x4, u64, u32, u32, u32, vp], ci),
        "fhe_bit_reverse": ([vp, u32, u32, vp], ci),
        "fhe_sample_uniform_lcg": ([vp, U64x4, u64, sz, vp], ci),
        "fhe_sample_gaussian_placeholder": ([vp, U64x4, u64, sz, vp], ci),
        "fhe_rns_sample_ternary": ([vp, vp, ctypes.c_double, u64, u32], ci),
        "fhe_rns_sample_gaussian": ([vp, vp, ctypes.c_double, u64, u32], ci),
        "fhe_rns_sample_uniform": ([vp, vp, u64, u32], ci),
        "fhe_gaussian_cdt": ([ctypes.c_double, P(u64), u32, P(u32)], ci),
        "fhe_poly_mod_switch": ([vp, vp, U64x4, U64x4, sz, vp], ci),
        "fhe_negacyclic_reduce": ([vp, U64x4, sz, vp], ci),
        "fhe_rns_rescale_drop_last": ([vp, vp, vp, u32], ci),
        "fhe_ct_mod_switch_drop_last": ([vp, u64, P(vp), P(vp), u32, u32], ci),
        "fhe_relin_num_digits": ([vp, u32, P(u32)], ci),
        "fhe_relin_keys_create": ([vp, P(vp), u32, P(vp), P(vp), u32], ci),
        "fhe_relin_keys_destroy": ([vp], ci),
        "fhe_ct_relinearize": ([vp, vp, vp, vp, vp, u32], ci),
        "fhe_ct_multiply_relin": ([vp, vp, vp, vp, vp, vp, vp, vp, u32], ci),
        "fhe_galois_element": ([u32, ctypes.c_int32, P(u32)], ci),
        "fhe_rns_automorphism": ([vp, vp, vp, u32, u32], ci),
        "fhe_ct_apply_galois": ([vp, vp, u32, vp, vp, vp, vp, u32], ci),
        "fhe_ct_hoist": ([vp, u32, vp, u32], ci),
        "fhe_ct_apply_galois_hoisted": ([vp, vp, u32, vp, vp, vp, u32], ci),
        "fhe_rns_ntt_reserve_hoist": ([vp, u32, u32], ci),
        "fhe_rns_ntt_hoist_bytes": ([vp, ctypes.POINTER(ctypes.c_uint64)], ci),
        "fhe_linear_transform_create": ([vp, P(vp), u32, P(u32), P(vp), P(vp), u32], ci),
        "fhe_linear_transform_destroy": ([vp], ci),
        "fhe_linear_transform_reserve": ([vp, vp, u32], ci),
        "fhe_ct_linear_transform_hoisted": ([vp, vp, vp, vp, vp, vp, u32], ci),
        "fhe_public_key_create": ([vp, P(vp), vp, vp], ci),
        "fhe_public_key_destroy": ([vp], ci),
        "fhe_ct_encrypt_reserve": ([vp, ctypes.c_double, u32], ci),
        "fhe_ct_encrypt": ([vp, vp, u64, ctypes.c_double, P(u64), vp, vp, vp, u32], ci),
        "fhe_secret_key_create": ([vp, P(vp), vp], ci),
        "fhe_secret_key_destroy": ([vp], ci),
        "fhe_ct_decrypt_reserve": ([vp, u64, u32, u32], ci),
        "fhe_ct_decrypt": ([vp, vp, u64, u64, vp, vp, P(vp), u32, u32], ci),
        "fhe_keyswitch_keys_generate": ([vp, vp, u32, P(u32), u32, u64, ctypes.c_double, P(u64), P(vp)], ci),
        "fhe_relin_keys_export": ([vp, vp, vp, vp], ci),
        "fhe_rgsw_keys_generate": ([vp, vp, u32, P(ctypes.c_int32), u32, u64, ctypes.c_double, P(u64), P(vp), P(vp)], ci),
        "fhe_lwe_prepare_accumulator": ([vp, u64, u32, vp, vp, vp, vp, vp, u32], ci),
        "fhe_rlwe_sample_extract": ([vp, vp, vp, vp, u32, u32], ci),
        "fhe_rlwe_sample_extract_strided": ([vp, vp, vp, vp, u32, u32], ci),
        "fhe_lwe_ksk_num_digits": ([vp, u32, P(u32)], ci),
        "fhe_lwe_ksk_create": ([vp, P(vp), u32, u32, vp], ci),
        "fhe_lwe_ksk_export": ([vp, vp, vp], ci),
        "fhe_lwe_ksk_destroy": ([vp], ci),
        "fhe_lwe_ksk_bytes": ([vp, P(u64)], ci),
        "fhe_lwe_ksk_generate": ([vp, vp, u32, u32, P(ctypes.c_int32), u64, ctypes.c_double, P(u64), P(vp)], ci),
        "fhe_lwe_keyswitch": ([vp, vp, u64, vp, vp, u32], ci),
        "fhe_lwe_pack_galois_elements": ([u32, P(u32)], ci),
        "fhe_lwe_to_rlwe": ([vp, vp, vp, vp, u32], ci),
        "fhe_lwe_pack": ([vp, P(vp), vp, vp, vp, u32, ci, ci, u32], ci),
        "fhe_lwe_pack_reserve": ([vp, P(vp), u32, ci, u32], ci),
        "fhe_rlwe_pack": ([vp, P(vp), vp, vp, vp, vp, u32, ci, ci, u32], ci),
        "fhe_batch_encoder_create": ([vp, P(vp), u64, ci], ci),
        "fhe_batch_encoder_destroy": ([vp], ci),
        "fhe_batch_encoder_reserve": ([vp, vp, u32], ci),
        "fhe_batch_encoder_scratch_bytes": ([vp, P(u64)], ci),
        "fhe_batch_encoder_slot_table": ([u32, ci, P(u32)], ci),
        "fhe_slots_encode": ([vp, vp, vp, vp, u32], ci),
        "fhe_slots_decode": ([vp, vp, vp, vp, u32], ci),
        "fhe_slots_decode_poly": ([vp, vp, vp, vp, u32], ci),
        "fhe_ckks_encoder_create": ([vp, P(vp)], ci),
        "fhe_ckks_encoder_destroy": ([vp], ci),
        "fhe_ckks_slot_table": ([u32, P(u32), P(ctypes.c_uint8)], ci),
        "fhe_ckks_encode": ([vp, vp, vp, vp, vp, ctypes.c_double, u32], ci),
        "fhe_ckks_decode": ([vp, vp, vp, vp, u64, ctypes.c_double, u32], ci),
        "fhe_ckks_decode_poly": ([vp, vp, vp, vp, ctypes.c_double, u32], ci),
        "fhe_bfv_multiplier_create": ([vp, P(vp), u64, P(u64), u32], ci),
        "fhe_bfv_multiplier_destroy": ([vp], ci),
        "fhe_bfv_multiplier_engine": ([vp, P(vp)], ci),
        "fhe_bfv_multiplier_reserve": ([vp, u32, vp], ci),
        "fhe_bfv_multiplier_workspace_bytes": ([vp, P(u64)], ci),
        "fhe_bfv_lift": ([vp, vp, vp, u32], ci),
        "fhe_bfv_scale_round": ([vp, P(vp), P(vp), u32, u32], ci),
        "fhe_bfv_multiply": ([vp, vp, vp, vp, vp, vp, vp, vp, u32], ci),
        "fhe_bfv_multiply_relin": ([vp, vp, vp, vp, vp, vp, vp, vp, u32], ci),
        "fhe_timer_create": ([P(vp)], ci),
        "fhe_timer_destroy": ([vp], ci),
        "fhe_rns_timer_start": ([vp, vp], ci),
        "fhe_rns_timer_stop": ([vp, vp], ci),
        "fhe_timer_elapsed_ms": ([vp, P(ctypes.c_float)], ci),
    }
    for name, (args, res) in sigs.items():
        fn = getattr(L, name)          # AttributeError here == the library does not export a declared symbol
        fn.argtypes, fn.restype = args, res
    L._fhe_symbols = sorted(sigs)
    _lib = L
    return L


def _check(rc):
    if rc != 0:
        raise FheError(rc, lib().fhe_hip_last_error().decode(errors="replace"))


def _q4(q):
    return U64x4(*[(int(q) >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)])


def _int(v):
    return sum(int(v[i]) << (64 * i) for i in range(4))


# ---- host-side parameter maths (works without a GPU) -------------------------------------------
def montgomery_inverse(q):
    out = U64x4(); _check(lib().fhe_montgomery_inverse(_q4(q), out)); return _int(out)


def montgomery_params(q):
    r2, inv = U64x4(), U64x4(); _check(lib().fhe_montgomery_params(_q4(q), r2, inv)); return _int(r2), _int(inv)


def find_ntt_primes(bits, n, count):
    if bits > 64:
        out = (U64x4 * count)(); _check(lib().fhe_find_ntt_primes_wide(bits, n, count, ctypes.cast(out, ctypes.c_void_p)))
        return [_int(x) for x in out]
    out = (ctypes.c_uint64 * count)(); _check(lib().fhe_find_ntt_primes(bits, n, count, out)); return [int(x) for x in out]


def find_psi(n, q):
    out = U64x4(); _check(lib().fhe_find_psi(n, _q4(q), out)); return _int(out)


def galois_element(n, steps):
    """3^(steps mod n/2) mod 2n: the Galois element of a row rotation by `steps` slots (host only)."""
    e = ctypes.c_uint32(0); _check(lib().fhe_galois_element(n, steps, ctypes.byref(e))); return e.value


def lwe_pack_galois_elements(n):
    """[2^j + 1 for j = 1 .. log2 n]: the Galois elements whose keys fhe_lwe_pack takes, in the order of its key array (host only)."""
    if not 0 < int(n) < 1 << 32:
        raise FheError(-1, "lwe_pack_galois_elements: n must be a power of two in [8, 2^30]")
    out = (ctypes.c_uint32 * 32)(); _check(lib().fhe_lwe_pack_galois_elements(n, out)); return [int(out[j]) for j in range(int(n).bit_length() - 1)]


def device_count():
    c = ctypes.c_int(0)
    rc = lib().fhe_hip_device_count(ctypes.byref(c))
    return c.value if rc == 0 else 0


def device_name():
    buf = ctypes.create_string_buffer(256); _check(lib().fhe_hip_device_name(buf, 256)); return buf.value.decode()


def sync():
    _check(lib().fhe_hip_sync())


# ---- device memory --------------------------------------------------------------------------------
class DeviceBuffer:
    """hipMalloc'd buffer of 256-bit containers; host view = numpy uint64 (..., 4)."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        p = ctypes.c_void_p()
        _check(lib().fhe_hip_malloc(ctypes.byref(p), self.nbytes))
        self.ptr = p.value

    @classmethod
    def from_numpy(cls, arr):
        arr = np.ascontiguousarray(arr)
        b = cls(arr.nbytes); b.upload(arr); return b

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        _check(lib().fhe_hip_memcpy_h2d(self.ptr, arr.ctypes.data, arr.nbytes))

    def download(self, shape=None, dtype=np.uint64):
        out = np.empty(self.nbytes // np.dtype(dtype).itemsize, dtype=dtype)
        _check(lib().fhe_hip_sync())      # engines enqueue asynchronously; callers synchronise (tests/test_fhe.cu:88)
        _check(lib().fhe_hip_memcpy_d2h(out.ctypes.data, self.ptr, self.nbytes))
        return out.reshape(shape) if shape is not None else out.reshape(-1, 4)

    def zero(self):
        _check(lib().fhe_hip_memset(self.ptr, 0, self.nbytes))

    def free(self):
        if getattr(self, "ptr", None):
            lib().fhe_hip_free(self.ptr); self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _ptr(x):
    if isinstance(x, DeviceBuffer):
        return x.ptr
    if hasattr(x, "data_ptr"):           # torch tensor on the GPU
        return x.data_ptr()
    return int(x)


# ---- literal element-wise primitives ----------------------------------------------------------------
def ref_forward_kernel_literal(data, twiddles, q, inv0, n, batch=1, stream=None):
    _check(lib().fhe_ref_forward_kernel_literal(_ptr(data), _ptr(twiddles), _q4(q), inv0, n, batch, stream))


def ref_inverse_kernel_literal(data, inv_twiddles, q, inv0, n_inv, n, batch=1, stream=None):
    _check(lib().fhe_ref_inverse_kernel_literal(_ptr(data), _ptr(inv_twiddles), _q4(q), inv0, _q4(n_inv), n, batch, stream))


def ref_stockham_stage_literal(output, data, twiddles, q, inv0, n, stage, batch=1, stream=None):
    _check(lib().fhe_ref_stockham_stage_literal(_ptr(output), _ptr(data), _ptr(twiddles), _q4(q), inv0, n, stage, batch, stream))


def bit_reverse(data, n, batch=1, stream=None):
    _check(lib().fhe_bit_reverse(_ptr(data), n, batch, stream))


def sample_uniform_lcg(out, q, seed, count, stream=None):
    _check(lib().fhe_sample_uniform_lcg(_ptr(out), _q4(q), seed, count, stream))


def sample_gaussian_placeholder(out, q, seed, count, stream=None):
    _check(lib().fhe_sample_gaussian_placeholder(_ptr(out), _q4(q), seed, count, stream))


def gaussian_cdt(sigma):
    n = ctypes.c_uint32(0); _check(lib().fhe_gaussian_cdt(sigma, None, 0, ctypes.byref(n)))
    t = (ctypes.c_uint64 * n.value)(); _check(lib().fhe_gaussian_cdt(sigma, t, n.value, ctypes.byref(n)))
    return [int(v) for v in t]


def poly_mod_switch(r, a, old_q, new_q, count, stream=None):
    _check(lib().fhe_poly_mod_switch(_ptr(r), _ptr(a), _q4(old_q), _q4(new_q), count, stream))


def negacyclic_reduce(data, q, n, stream=None):
    _check(lib().fhe_negacyclic_reduce(_ptr(data), _q4(q), n, stream))


def u256_add_mod(r, a, b, q, count, stream=None):
    _check(lib().fhe_u256_add_mod(_ptr(r), _ptr(a), _ptr(b), _q4(q), count, stream))


def u256_sub_mod(r, a, b, q, count, stream=None):
    _check(lib().fhe_u256_sub_mod(_ptr(r), _ptr(a), _ptr(b), _q4(q), count, stream))


def u256_mont_mul(r, a, b, q, inv0, count, stream=None):
    _check(lib().fhe_u256_mont_mul(_ptr(r), _ptr(a), _ptr(b), _q4(q), inv0, count, stream))


def u256_mont_mul_scalar(r, a, scalar, q, inv0, count, stream=None):
    _check(lib().fhe_u256_mont_mul_scalar(_ptr(r), _ptr(a), _q4(scalar), _q4(q), inv0, count, stream))


# ---- engines ------------------------------------------------------------------------------------------
class NttEngine:
    """fhe::NTTEngine (include/ntt.cuh:72-103)."""

    def __init__(self, n, q):
        self.h = None
        h = ctypes.c_void_p()
        _check(lib().fhe_ntt_create(ctypes.byref(h), n, _q4(q)))
        self.h, self.n, self.q = h, n, q

    @property
    def width_class(self):
        return lib().fhe_ntt_width_class(self.h)

    def set_stream(self, stream):
        _check(lib().fhe_ntt_set_stream(self.h, stream))

    def forward(self, d_data, batch=1):
        _check(lib().fhe_ntt_forward(self.h, _ptr(d_data), batch))

    def inverse(self, d_data, batch=1):
        _check(lib().fhe_ntt_inverse(self.h, _ptr(d_data), batch))

    def pointwise(self, d_r, d_a, d_b, batch=1):
        _check(lib().fhe_ntt_pointwise(self.h, _ptr(d_r), _ptr(d_a), _ptr(d_b), batch))

    def multiply(self, d_r, d_a, d_b, batch=1):
        _check(lib().fhe_ntt_multiply(self.h, _ptr(d_r), _ptr(d_a), _ptr(d_b), batch))

    def close(self):
        if self.h:
            lib().fhe_ntt_destroy(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RnsNttEngine:
    """fhe::RNS_NTTEngine (include/ntt.cuh:106-137) + the FHEContext::multiply tensor product."""

    def __init__(self, n, moduli):
        self.h = None
        L = len(moduli)
        arr = (U64x4 * L)(*[_q4(q) for q in moduli])
        h = ctypes.c_void_p()
        if n is None:                      # RNS base without a ring (RNSContext): degree-1 engine, buffers [count][L]
            _check(lib().fhe_rns_base_create(ctypes.byref(h), ctypes.cast(arr, ctypes.c_void_p), L)); n = 1
        else:
            _check(lib().fhe_rns_ntt_create(ctypes.byref(h), n, ctypes.cast(arr, ctypes.c_void_p), L))
        self.h, self.n, self.L, self.moduli, self.borrowed = h, n, L, list(moduli), False

    @classmethod
    def _borrow(cls, handle, n, moduli):
        """A view of an engine that another object owns (the extended engine of a BfvMultiplier): close() lets go of it without destroying it."""
        e = cls.__new__(cls)
        e.h, e.n, e.L, e.moduli, e.borrowed = handle, n, len(moduli), list(moduli), True
        return e

    @property
    def width_class(self):
        return lib().fhe_rns_ntt_width_class(self.h)

    def set_stream(self, stream):
        _check(lib().fhe_rns_ntt_set_stream(self.h, stream))

    def forward(self, d_data, batch=1):
        _check(lib().fhe_rns_ntt_forward(self.h, _ptr(d_data), batch))

    def inverse(self, d_data, batch=1):
        _check(lib().fhe_rns_ntt_inverse(self.h, _ptr(d_data), batch))

    def pointwise(self, d_r, d_a, d_b, batch=1):
        _check(lib().fhe_rns_ntt_pointwise(self.h, _ptr(d_r), _ptr(d_a), _ptr(d_b), batch))

    def multiply(self, d_r, d_a, d_b, batch=1):
        _check(lib().fhe_rns_ntt_multiply(self.h, _ptr(d_r), _ptr(d_a), _ptr(d_b), batch))

    def multiply_bcast(self, d_r, d_a, d_b_one, batch=1):
        _check(lib().fhe_rns_ntt_multiply_bcast(self.h, _ptr(d_r), _ptr(d_a), _ptr(d_b_one), batch))

    def poly_add(self, d_r, d_a, d_b, batch=1):
        _check(lib().fhe_rns_poly_add(self.h, _ptr(d_r), _ptr(d_a), _ptr(d_b), batch))

    def mul_mont_literal(self, d_r, d_a, d_b, batch=1):
        _check(lib().fhe_rns_mul_mont_literal(self.h, _ptr(d_r), _ptr(d_a), _ptr(d_b), batch))

    def poly_sub(self, d_r, d_a, d_b, batch=1):
        _check(lib().fhe_rns_poly_sub(self.h, _ptr(d_r), _ptr(d_a), _ptr(d_b), batch))

    def ct_multiply(self, d_c0, d_c1, d_c2, d_a0, d_a1, d_b0, d_b1, batch=1):
        _check(lib().fhe_ct_multiply(self.h, _ptr(d_c0), _ptr(d_c1), _ptr(d_c2), _ptr(d_a0), _ptr(d_a1), _ptr(d_b0),
                                     _ptr(d_b1), batch))

    def to_rns(self, d_rns, d_values, batch=1):
        _check(lib().fhe_rns_to_rns(self.h, _ptr(d_rns), _ptr(d_values), batch))

    def from_rns(self, d_values, d_rns, batch=1):
        _check(lib().fhe_rns_from_rns(self.h, _ptr(d_values), _ptr(d_rns), batch))

    def monomial_mul_sub(self, d_out, d_in, d_shifts, batch=1):
        _check(lib().fhe_rns_monomial_mul_sub(self.h, _ptr(d_out), _ptr(d_in), _ptr(d_shifts), batch))

    def blind_rotate_step(self, rows_c0, rows_c1, d_acc0, d_acc1, d_shifts, d_tmp0, d_tmp1, batch=1):
        _check(lib().fhe_blind_rotate_step(self.h, rows_c0.h, rows_c1.h, _ptr(d_acc0), _ptr(d_acc1), _ptr(d_shifts), _ptr(d_tmp0),
                                           _ptr(d_tmp1), batch))

    def blind_rotate(self, rows_c0, rows_c1, d_acc0, d_acc1, d_shifts, d_tmp0, d_tmp1, batch=1):
        """rows_c0 / rows_c1: one imported row set per step (lists of equal length); d_shifts: device uint32 [steps][batch]."""
        steps = len(rows_c0); assert len(rows_c1) == steps
        arr = ctypes.c_void_p * max(steps, 1)
        a0 = arr(*[r.h for r in rows_c0]); a1 = arr(*[r.h for r in rows_c1])
        _check(lib().fhe_blind_rotate(self.h, a0, a1, steps, _ptr(d_acc0), _ptr(d_acc1), _ptr(d_shifts), _ptr(d_tmp0), _ptr(d_tmp1), batch))

    def sample_ternary(self, d_out, probability, seed, batch=1):
        _check(lib().fhe_rns_sample_ternary(self.h, _ptr(d_out), probability, seed, batch))

    def sample_gaussian(self, d_out, sigma, seed, batch=1):
        _check(lib().fhe_rns_sample_gaussian(self.h, _ptr(d_out), sigma, seed, batch))

    def sample_uniform(self, d_out, seed, batch=1):
        _check(lib().fhe_rns_sample_uniform(self.h, _ptr(d_out), seed, batch))

    def fast_base_convert(self, target, d_out, d_in, batch=1):
        _check(lib().fhe_rns_fast_base_convert(self.h, target.h, _ptr(d_out), _ptr(d_in), batch))

    def rescale_drop_last(self, d_out, d_in, batch=1):
        _check(lib().fhe_rns_rescale_drop_last(self.h, _ptr(d_out), _ptr(d_in), batch))

    def ct_mod_switch(self, t, outs, ins, batch=1):
        """BGV modulus switch: drops the last prime from the components `ins` ([batch][L][n] each) into `outs` ([batch][L-1][n]), one launch;
        the plaintext modulo t is kept up to the factor q_last^-1 mod t."""
        k = len(ins)
        arr = lambda xs: (ctypes.c_void_p * max(len(xs), 1))(*[None if x is None else _ptr(x) for x in xs])   # None: a null pointer (rejected)
        po, pi = arr(outs), arr(ins)
        _check(lib().fhe_ct_mod_switch_drop_last(self.h, t, po, pi, k, batch))

    def relin_num_digits(self, decomp_bits):
        k = ctypes.c_uint32(0); _check(lib().fhe_relin_num_digits(self.h, decomp_bits, ctypes.byref(k))); return k.value

    def import_relin_keys(self, decomp_bits, keys_b, keys_a):
        """keys_b / keys_a: lists of device buffers, each an [L][n] polynomial in coefficient form."""
        n = len(keys_b)
        pb = (ctypes.c_void_p * n)(*[_ptr(k) for k in keys_b]); pa = (ctypes.c_void_p * n)(*[_ptr(k) for k in keys_a])
        out = ctypes.c_void_p()
        _check(lib().fhe_relin_keys_create(self.h, ctypes.byref(out), decomp_bits, pb, pa, n))
        return RelinKeys(out)

    def relinearize(self, rk, d_c0, d_c1, d_c2, batch=1):
        _check(lib().fhe_ct_relinearize(self.h, rk.h, _ptr(d_c0), _ptr(d_c1), _ptr(d_c2), batch))

    def reserve(self, batch):
        """Pre-size the library workspaces for calls of up to `batch` units (needed before hipGraph capture)."""
        _check(lib().fhe_rns_ntt_reserve(self.h, batch))

    def workspace_bytes(self):
        """Device bytes the engine's library-owned workspaces hold right now."""
        out = ctypes.c_uint64(0)
        _check(lib().fhe_rns_ntt_workspace_bytes(self.h, ctypes.byref(out)))
        return out.value

    def ct_multiply_relin(self, rk, d_c0, d_c1, d_a0, d_a1, d_b0, d_b1, batch=1):
        """FHEContext::multiply: tensor product + relinearisation in one call (two components out)."""
        _check(lib().fhe_ct_multiply_relin(self.h, rk.h, _ptr(d_c0), _ptr(d_c1), _ptr(d_a0), _ptr(d_a1), _ptr(d_b0), _ptr(d_b1), batch))

    def automorphism(self, d_out, d_in, galois_elt, batch=1):
        """d_out = sigma_g(d_in): a(x) -> a(x^g) per limb polynomial, g odd and below 2n (out of place)."""
        _check(lib().fhe_rns_automorphism(self.h, _ptr(d_out), _ptr(d_in), galois_elt, batch))

    def apply_galois(self, gk, galois_elt, d_out0, d_out1, d_c0, d_c1, batch=1):
        """(d_out0, d_out1) = sigma_g applied to the ciphertext (d_c0, d_c1) and key-switched back with the Galois keys gk of g
        (imported with import_relin_keys: rows (b, a) with b = -a*s + e + g_jk * sigma_g(s))."""
        _check(lib().fhe_ct_apply_galois(self.h, gk.h, galois_elt, _ptr(d_out0), _ptr(d_out1), _ptr(d_c0), _ptr(d_c1), batch))

    def hoist(self, decomp_bits, d_c1, batch=1):
        """Decompose and transform c1 once; the engine keeps the result for apply_galois_hoisted until the next hoist."""
        _check(lib().fhe_ct_hoist(self.h, decomp_bits, _ptr(d_c1), batch))

    def apply_galois_hoisted(self, gk, galois_elt, d_out0, d_out1, d_c0, batch=1):
        """One rotation of the hoisted ciphertext: d_c0 is the c0 that belongs to the hoisted c1, gk the Galois keys of g."""
        _check(lib().fhe_ct_apply_galois_hoisted(self.h, gk.h, galois_elt, _ptr(d_out0), _ptr(d_out1), _ptr(d_c0), batch))

    def reserve_hoist(self, decomp_bits, batch):
        """Pre-size the hoist workspace (and what the two calls need of the others) so that neither allocates afterwards."""
        _check(lib().fhe_rns_ntt_reserve_hoist(self.h, decomp_bits, batch))

    def hoist_bytes(self):
        """Device bytes of the hoist workspace (not counted by workspace_bytes)."""
        out = ctypes.c_uint64(0)
        _check(lib().fhe_rns_ntt_hoist_bytes(self.h, ctypes.byref(out)))
        return out.value

    def linear_transform_create(self, decomp_bits, galois_elts, keys, plains):
        """sum_t plains[t] * rotation by galois_elts[t]: keys[t] the Galois keys of that element (None with element 1: no key switch),
        plains[t] one [L][n] polynomial in coefficient form on the device.  The key sets are referenced and must outlive the object."""
        G = len(galois_elts); assert len(keys) == G and len(plains) == G
        m = max(G, 1)
        elts = (ctypes.c_uint32 * m)(*galois_elts)
        pk = (ctypes.c_void_p * m)(*[None if k is None else k.h for k in keys])
        pp = (ctypes.c_void_p * m)(*[None if p is None else _ptr(p) for p in plains])
        out = ctypes.c_void_p()
        _check(lib().fhe_linear_transform_create(self.h, ctypes.byref(out), decomp_bits, elts, pk, pp, G))
        return LinearTransform(out, list(keys))

    def linear_transform_reserve(self, lt, batch):
        """Pre-size what linear_transform_hoisted (and the hoist before it) needs for `batch` ciphertexts: reserve, then hoist."""
        _check(lib().fhe_linear_transform_reserve(self.h, lt.h, batch))

    def linear_transform_hoisted(self, lt, d_out0, d_out1, d_c0, d_c1=None, batch=1):
        """(d_out0, d_out1) = sum_t p_t * rotation_t of the hoisted ciphertext; d_c1 is needed only when lt has a keyless term."""
        _check(lib().fhe_ct_linear_transform_hoisted(self.h, lt.h, _ptr(d_out0), _ptr(d_out1), _ptr(d_c0), None if d_c1 is None else _ptr(d_c1), batch))

    def import_public_key(self, d_pk0, d_pk1):
        """(pk0, pk1): one [L][n] polynomial each, coefficient form, on the device.  The library keeps its own copies."""
        out = ctypes.c_void_p()
        _check(lib().fhe_public_key_create(self.h, ctypes.byref(out), _ptr(d_pk0), _ptr(d_pk1)))
        return PublicKey(out)

    def encrypt_reserve(self, sigma, batch):
        """Pre-size what encrypt needs for this sigma and up to `batch` ciphertexts: afterwards a call allocates nothing."""
        _check(lib().fhe_ct_encrypt_reserve(self.h, sigma, batch))

    def encrypt(self, pk, t, sigma, seeds, d_out0, d_out1, d_m=None, batch=1):
        """(d_out0, d_out1) = (pk0 * u + t e0 + m, pk1 * u + t e1) for `batch` ciphertexts; seeds = (u, e0, e1); d_m None encrypts zero."""
        assert len(seeds) == 3
        sd = (ctypes.c_uint64 * 3)(*[int(x) & 0xFFFFFFFFFFFFFFFF for x in seeds])
        _check(lib().fhe_ct_encrypt(self.h, pk.h, t, sigma, sd, _ptr(d_out0), _ptr(d_out1), None if d_m is None else _ptr(d_m), batch))

    def import_secret_key(self, d_s):
        """s: one [L][n] polynomial, coefficient form, on the device.  The library keeps its own copy (and s * s)."""
        out = ctypes.c_void_p()
        _check(lib().fhe_secret_key_create(self.h, ctypes.byref(out), _ptr(d_s)))
        return SecretKey(out)

    def decrypt_reserve(self, t, num_components, batch):
        """Pre-size what decrypt needs for up to `num_components` components and `batch` ciphertexts: afterwards a call allocates nothing."""
        _check(lib().fhe_ct_decrypt_reserve(self.h, t, num_components, batch))

    def decrypt(self, sk, t, scale, d_m, d_noise_bits, components, batch=1):
        """d_m[b][x] = ((v mod t) * scale) mod t (uint64) and d_noise_bits[b] = bit_length(max |v|) (uint32, or None), v the centred value of
        c0 + c1 s (+ c2 s^2) for the 2 or 3 device buffers in `components`."""
        comps = (ctypes.c_void_p * len(components))(*[_ptr(c) for c in components])
        _check(lib().fhe_ct_decrypt(self.h, sk.h, t, scale, _ptr(d_m), None if d_noise_bits is None else _ptr(d_noise_bits), comps, len(components), batch))

    def generate_keyswitch_keys(self, sk, decomp_bits, elts, noise_scale, sigma, seeds):
        """One key set per entry of `elts` (0: relinearisation key; odd g below 2n: Galois key of g), generated on the device from the secret
        key `sk` with seeds = (a, e).  Returns the key-set objects, as import_relin_keys would for the same rows."""
        k = len(elts)
        ge = (ctypes.c_uint32 * max(k, 1))(*[int(g) for g in elts])
        sd = (ctypes.c_uint64 * 2)(*[int(x) & 0xFFFFFFFFFFFFFFFF for x in seeds])
        outs = (ctypes.c_void_p * max(k, 1))()
        _check(lib().fhe_keyswitch_keys_generate(self.h, sk.h, decomp_bits, ge, k, noise_scale, sigma, sd, outs))
        return [RelinKeys(ctypes.c_void_p(outs[i])) for i in range(k)]

    def generate_rgsw_keys(self, sk, decomp_bits, mu, noise_scale, sigma, seeds):
        """One RGSW ciphertext per entry of `mu` (small integers, |mu| <= 2^15), generated on the device from `sk` with seeds = (a, e).
        Returns (rows_c0, rows_c1), two lists of key-set objects as fhe_blind_rotate takes them."""
        k = len(mu)
        ms = (ctypes.c_int32 * max(k, 1))(*[int(m) for m in mu])
        sd = (ctypes.c_uint64 * 2)(*[int(x) & 0xFFFFFFFFFFFFFFFF for x in seeds])
        o0, o1 = (ctypes.c_void_p * max(k, 1))(), (ctypes.c_void_p * max(k, 1))()
        _check(lib().fhe_rgsw_keys_generate(self.h, sk.h, decomp_bits, ms, k, noise_scale, sigma, sd, o0, o1))
        return [RelinKeys(ctypes.c_void_p(o0[i])) for i in range(k)], [RelinKeys(ctypes.c_void_p(o1[i])) for i in range(k)]

    def lwe_prepare_accumulator(self, q_lwe, n_lwe, d_lwe, d_tv, d_acc0, d_acc1, d_shifts, batch=1):
        """d_lwe: device uint64 [batch][n_lwe + 1] -> acc0 = X^(2n - ms(b)) tv, acc1 = 0, d_shifts = device uint32 [n_lwe][batch]."""
        _check(lib().fhe_lwe_prepare_accumulator(self.h, q_lwe, n_lwe, _ptr(d_lwe), _ptr(d_tv), _ptr(d_acc0), _ptr(d_acc1), _ptr(d_shifts), batch))

    def sample_extract(self, d_out, d_c0, d_c1, idx, batch=1):
        """Coefficient idx of (c0, c1) as LWE samples: d_out = device uint64 [batch][L][n + 1]."""
        _check(lib().fhe_rlwe_sample_extract(self.h, _ptr(d_out), _ptr(d_c0), _ptr(d_c1), idx, batch))

    def sample_extract_strided(self, d_out, d_c0, d_c1, count, batch=1):
        """Coefficients i n / count, i < count, of (c0, c1) as LWE samples in one launch: d_out = device uint64 [batch][count][L][n + 1], row
        (b, i, l) what sample_extract writes at idx = i n / count.  The d_lwe of lwe_pack; on a one-limb engine the d_in of lwe_keyswitch."""
        _check(lib().fhe_rlwe_sample_extract_strided(self.h, _ptr(d_out), _ptr(d_c0), _ptr(d_c1), count, batch))

    lwe_pack_galois_elements = staticmethod(lwe_pack_galois_elements)

    def lwe_to_rlwe(self, d_c0, d_c1, d_lwe, batch=1):
        """The RLWE embedding of LWE samples under the ring key: d_lwe = device uint64 [batch][L][n + 1] -> (d_c0, d_c1) [batch][L][n] containers,
        the inverse of sample_extract at idx = 0."""
        _check(lib().fhe_lwe_to_rlwe(self.h, _ptr(d_c0), _ptr(d_c1), _ptr(d_lwe), batch))

    @staticmethod
    def _pack_keys(keys):
        return (ctypes.c_void_p * max(len(keys), 1))(*[None if k is None else k.h for k in keys])

    def lwe_pack(self, keys, d_out0, d_out1, d_lwe, count, trace=True, normalize=True, batch=1):
        """d_lwe = device uint64 [batch][count][L][n + 1] -> one RLWE ciphertext per batch element whose coefficient i (n / count) carries the
        phase of sample i.  keys[j - 1]: the Galois keys of 2^j + 1 (lwe_pack_galois_elements), None where the call does not use them."""
        _check(lib().fhe_lwe_pack(self.h, self._pack_keys(keys), _ptr(d_out0), _ptr(d_out1), _ptr(d_lwe), count, int(bool(trace)), int(bool(normalize)), batch))

    def lwe_pack_reserve(self, keys, count, trace=True, batch=1):
        """Pre-size what lwe_pack needs for this shape (its own scratch and the key switch's): afterwards a call allocates nothing."""
        _check(lib().fhe_lwe_pack_reserve(self.h, self._pack_keys(keys), count, int(bool(trace)), batch))

    def rlwe_pack(self, keys, d_out0, d_out1, d_c0, d_c1, count, trace=True, normalize=True, batch=1):
        """lwe_pack of coefficient 0 of batch * count RLWE pairs, (d_c0, d_c1) = [batch][count][L][n] containers as blind_rotate leaves them,
        without the samples in between: the bits of sample_extract(idx = 0) + lwe_pack.  lwe_pack_reserve sizes the scratch of both."""
        _check(lib().fhe_rlwe_pack(self.h, self._pack_keys(keys), _ptr(d_out0), _ptr(d_out1), _ptr(d_c0), _ptr(d_c1), count, int(bool(trace)),
                                   int(bool(normalize)), batch))

    def lwe_ksk_num_digits(self, decomp_bits):
        """K = ceil(bit_length(q_0) / decomp_bits): the LWE key-switching key of this engine has n K rows."""
        k = ctypes.c_uint32(0); _check(lib().fhe_lwe_ksk_num_digits(self.h, decomp_bits, ctypes.byref(k))); return k.value

    def import_lwe_ksk(self, decomp_bits, n_out, d_rows):
        """d_rows: device uint64 [n K][n_out + 1], row j K + k = (a_0 .. a_{n_out-1}, b) encrypting s_j 2^(k w) under z.  Copied."""
        out = ctypes.c_void_p()
        _check(lib().fhe_lwe_ksk_create(self.h, ctypes.byref(out), decomp_bits, n_out, _ptr(d_rows)))
        return LweKeySwitchKey(out, n_out)

    def generate_lwe_ksk(self, sk, decomp_bits, z, noise_scale, sigma, seeds):
        """The LWE key-switching key from the ring key `sk` (limb 0) to the small key z (integers, |z_i| <= 2^15), generated on the device
        with seeds = (a, e).  Returns the key object, as import_lwe_ksk would for the same table."""
        k = len(z)
        zs = (ctypes.c_int32 * max(k, 1))(*[int(v) for v in z])
        sd = (ctypes.c_uint64 * 2)(*[int(x) & 0xFFFFFFFFFFFFFFFF for x in seeds])
        out = ctypes.c_void_p()
        _check(lib().fhe_lwe_ksk_generate(self.h, sk.h, decomp_bits, k, zs, noise_scale, sigma, sd, ctypes.byref(out)))
        return LweKeySwitchKey(out, k)

    def export_lwe_ksk(self, ksk, d_rows):
        """The canonical table [n K][n_out + 1] of any LWE key-switching key (the inverse of import_lwe_ksk)."""
        _check(lib().fhe_lwe_ksk_export(self.h, ksk.h, _ptr(d_rows)))

    def lwe_keyswitch(self, ksk, d_out, d_in, q_out=0, batch=1):
        """d_in: device uint64 [batch][n + 1] under the ring key -> d_out [batch][n_out + 1] under the small key; q_out != 0 also switches
        the modulus to q_out (at most 2^48) with rounding."""
        _check(lib().fhe_lwe_keyswitch(self.h, ksk.h, q_out, _ptr(d_out), _ptr(d_in), batch))

    def export_keys(self, rk, d_keys_b, d_keys_a):
        """The rows of any key set as [L*K][L][n] canonical containers in coefficient form (the inverse of import_relin_keys)."""
        _check(lib().fhe_relin_keys_export(self.h, rk.h, _ptr(d_keys_b), _ptr(d_keys_a)))

    def check_canonical(self, d_data, batch=1):
        _check(lib().fhe_rns_check_canonical(self.h, _ptr(d_data), batch))

    def close(self):
        if self.h:
            if not self.borrowed:                         # (the extended engine of a BfvMultiplier belongs to the multiplier)
                lib().fhe_rns_ntt_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RelinKeys:
    """Relinearisation keys imported into an engine (NTT-domain copies owned by the library)."""

    def __init__(self, h):
        self.h = h

    def close(self):
        if self.h:
            lib().fhe_relin_keys_destroy(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LweKeySwitchKey:
    """An LWE key-switching key (ring key -> small LWE key), owned by the library; bound to (n, q_0, device), not to one engine."""

    def __init__(self, h, n_out):
        self.h, self.n_out = h, n_out

    def nbytes(self):
        b = ctypes.c_uint64(0); _check(lib().fhe_lwe_ksk_bytes(self.h, ctypes.byref(b))); return b.value

    def close(self):
        if self.h:
            lib().fhe_lwe_ksk_destroy(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LinearTransform:
    """A hoisted linear transform built on an engine (plaintexts owned by the library; holds its key sets alive)."""

    def __init__(self, h, keys=()):
        self.h, self.keys = h, keys

    def close(self):
        if self.h:
            lib().fhe_linear_transform_destroy(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PublicKey:
    """A public key imported into an engine (copies owned by the library)."""

    def __init__(self, h):
        self.h = h

    def close(self):
        if self.h:
            lib().fhe_public_key_destroy(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SecretKey:
    """A secret key imported into an engine (copies owned by the library)."""

    def __init__(self, h):
        self.h = h

    def close(self):
        if self.h:
            lib().fhe_secret_key_destroy(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


SLOTS_NATURAL, SLOTS_ROWS = 0, 1


def slot_table(n, order):
    """The encoder's table, position of the NTT domain -> slot index, built on the host (no device needed): numpy uint32 [n]."""
    out = np.zeros(n, dtype=np.uint32)
    _check(lib().fhe_batch_encoder_slot_table(n, order, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))))
    return out


class BatchEncoder:
    """Slot values <-> plaintext polynomials of the engine `eng` for the plaintext modulus t (a prime = 1 mod 2n), on the device."""

    def __init__(self, eng, t, order=SLOTS_NATURAL):
        self.h = None
        self.eng = eng
        out = ctypes.c_void_p()
        _check(lib().fhe_batch_encoder_create(eng.h, ctypes.byref(out), t, order))
        self.h = out

    def reserve(self, batch):
        """Pre-size the encoder's scratch for up to `batch` plaintexts: afterwards no call allocates."""
        _check(lib().fhe_batch_encoder_reserve(self.eng.h, self.h, batch))

    def scratch_bytes(self):
        b = ctypes.c_uint64(0); _check(lib().fhe_batch_encoder_scratch_bytes(self.h, ctypes.byref(b))); return b.value

    def encode(self, d_out, d_values, batch=1):
        """d_out[b][l][x] = m_b[x] mod q_l ([batch][L][n] containers) for the [batch][n] uint64 slot values below t in d_values."""
        _check(lib().fhe_slots_encode(self.eng.h, self.h, _ptr(d_out), _ptr(d_values), batch))

    def decode(self, d_values, d_m, batch=1):
        """d_values[b][i] = m_b at slot i, for [batch][n] uint64 coefficients below t in d_m (what decrypt writes); d_values may be d_m."""
        _check(lib().fhe_slots_decode(self.eng.h, self.h, _ptr(d_values), _ptr(d_m), batch))

    def decode_poly(self, d_values, d_poly, batch=1):
        """The same from [batch][L][n] containers (limb 0 is read)."""
        _check(lib().fhe_slots_decode_poly(self.eng.h, self.h, _ptr(d_values), _ptr(d_poly), batch))

    def close(self):
        if self.h:
            lib().fhe_batch_encoder_destroy(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def ckks_slot_table(n):
    """(a(k), c(k)) of the CKKS slots k < n/2, built on the host (no device needed): numpy uint32 [n/2] and uint8 [n/2]."""
    a, c = np.zeros(max(n // 2, 1), dtype=np.uint32), np.zeros(max(n // 2, 1), dtype=np.uint8)
    _check(lib().fhe_ckks_slot_table(n, a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), c.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))))
    return a[:n // 2], c[:n // 2]


class CkksEncoder:
    """Complex slots <-> plaintext polynomials of the engine `eng` through the canonical embedding (FP64), on the device."""

    def __init__(self, eng):
        self.h = None
        self.eng = eng
        out = ctypes.c_void_p()
        _check(lib().fhe_ckks_encoder_create(eng.h, ctypes.byref(out)))
        self.h = out

    def encode(self, d_out, d_slots, scale, batch=1, d_coeff_bits=None):
        """d_out[b][l][j] = rne(scale m_b[j]) mod q_l ([batch][L][n] containers) for the [batch][n/2][2] doubles in d_slots; d_coeff_bits
        ([batch] uint32, optional) receives the bit length of the largest |coefficient|."""
        _check(lib().fhe_ckks_encode(self.eng.h, self.h, _ptr(d_out), None if d_coeff_bits is None else _ptr(d_coeff_bits), _ptr(d_slots), scale, batch))

    def decode(self, d_slots, d_m, t, scale, batch=1):
        """d_slots[b][k] = the slots of the [batch][n] uint64 words in d_m, centred modulo t (t = 0: two's complement), over scale."""
        _check(lib().fhe_ckks_decode(self.eng.h, self.h, _ptr(d_slots), _ptr(d_m), t, scale, batch))

    def decode_poly(self, d_slots, d_poly, scale, batch=1):
        """The same from [batch][L][n] containers (limb 0 is read, centred modulo q_0)."""
        _check(lib().fhe_ckks_decode_poly(self.eng.h, self.h, _ptr(d_slots), _ptr(d_poly), scale, batch))

    def close(self):
        if self.h:
            lib().fhe_ckks_encoder_destroy(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BfvMultiplier:
    """BFV multiplication on the engine `eng` (primes Q) for the plaintext modulus t: an extended engine on Q u P (P = the auxiliary NTT
    primes `aux_moduli`, of the same size as eng's, with P > 32 t n Q), the exact centred lift Q -> Q u P and scale-and-round by t / Q."""

    def __init__(self, eng, t, aux_moduli):
        self.h = None
        self.eng = eng
        aux = (ctypes.c_uint64 * max(len(aux_moduli), 1))(*[int(p) for p in aux_moduli])
        out = ctypes.c_void_p()
        _check(lib().fhe_bfv_multiplier_create(eng.h, ctypes.byref(out), t, aux, len(aux_moduli)))
        self.h, self.t, self.aux_moduli = out, t, [int(p) for p in aux_moduli]
        e = ctypes.c_void_p()
        _check(lib().fhe_bfv_multiplier_engine(self.h, ctypes.byref(e)))
        self._qp = RnsNttEngine._borrow(e, eng.n, list(eng.moduli) + self.aux_moduli)

    @property
    def engine(self):
        """The borrowed engine on Q u P (valid while the multiplier lives): tensor products of your own, scaled once by scale_round."""
        return self._qp

    def reserve(self, batch, rk=None):
        """Pre-size every workspace of multiply (and, with a key set, multiply_relin) for up to `batch` ciphertexts: afterwards no call allocates."""
        _check(lib().fhe_bfv_multiplier_reserve(self.h, batch, None if rk is None else rk.h))

    def workspace_bytes(self):
        b = ctypes.c_uint64(0); _check(lib().fhe_bfv_multiplier_workspace_bytes(self.h, ctypes.byref(b))); return b.value

    def lift(self, d_out, d_in, batch=1):
        """[batch][L][n] -> [batch][L + L'][n]: the Q limbs copied, the P limbs from the centred lift."""
        _check(lib().fhe_bfv_lift(self.h, _ptr(d_out), _ptr(d_in), batch))

    def scale_round(self, outs, ins, batch=1):
        """round(t x / Q) of 1 to 3 components `ins` ([batch][L + L'][n] each) into `outs` ([batch][L][n]), one launch."""
        arr = lambda xs: (ctypes.c_void_p * max(len(xs), 1))(*[None if x is None else _ptr(x) for x in xs])   # None: a null pointer (rejected)
        po, pi = arr(outs), arr(ins)
        _check(lib().fhe_bfv_scale_round(self.h, po, pi, len(ins), batch))

    def multiply(self, d_c0, d_c1, d_c2, d_a0, d_a1, d_b0, d_b1, batch=1):
        """(c0, c1, c2) = round(t / Q (a (x) b)) with the tensor product over the integers."""
        _check(lib().fhe_bfv_multiply(self.h, _ptr(d_c0), _ptr(d_c1), _ptr(d_c2), _ptr(d_a0), _ptr(d_a1), _ptr(d_b0), _ptr(d_b1), batch))

    def multiply_relin(self, rk, d_c0, d_c1, d_a0, d_a1, d_b0, d_b1, batch=1):
        """multiply followed by the relinearisation of c2 with the key set rk of eng: two components out."""
        _check(lib().fhe_bfv_multiply_relin(self.h, rk.h, _ptr(d_c0), _ptr(d_c1), _ptr(d_a0), _ptr(d_a1), _ptr(d_b0), _ptr(d_b1), batch))

    def close(self):
        if self.h:
            self._qp.h = None
            lib().fhe_bfv_multiplier_destroy(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Timer:
    """hipEvent pair recorded on an RnsNttEngine's stream."""

    def __init__(self):
        self.t = None
        t = ctypes.c_void_p(); _check(lib().fhe_timer_create(ctypes.byref(t))); self.t = t

    def start(self, eng):
        _check(lib().fhe_rns_timer_start(eng.h, self.t))

    def stop(self, eng):
        _check(lib().fhe_rns_timer_stop(eng.h, self.t))

    def elapsed_ms(self):
        ms = ctypes.c_float(0); _check(lib().fhe_timer_elapsed_ms(self.t, ctypes.byref(ms))); return ms.value

    def __del__(self):
        try:
            if self.t:
                lib().fhe_timer_destroy(self.t); self.t = None
        except Exception:
            pass
