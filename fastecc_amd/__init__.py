"""fastecc_amd — MI355X-native NTT Reed-Solomon encode path (FastECC-compatible).

Host-side Python harness over the C ABI of ``fastecc_amd/lib/libfastecc_hip.so`` (include/fastecc.h).
The product is the shared library; this module only binds it with ctypes so that tests and bench.py can
call exactly the entry points a C++ host (fastecc_amd/host/rs_main.cpp, or FastECC's RS.cpp patched as
in INTEGRATION.md) calls.  torch is used by callers for device memory and streams only — no torch type
appears in any signature here, just integer addresses.

There is no CPU compute path in this package: if the HIP library is missing or no GPU is present the
calls raise.
"""
import ctypes
import os

from . import _build

P = 0xFFF00001  # RS.cpp:86
P61 = (1 << 61) - 1
FIELD_GF_FFF00001 = 0
FIELD_GF_P61_SQUARED = 1  # GF((2^61-1)^2), 16-byte elements (re, im): include/fastecc.h
MEM_HOST, MEM_DEVICE, MEM_HOST_PINNED = 0, 1, 2
CODE_MIXED_RADIX = 1  # fastecc_create_ex flag: transform order q * 2^m, q in {1, 3, 5, 7, 9, 13, 15}
CODE_MIXED_RADIX_PFA = 4  # ... and the composite q = 21, 35, 39, 45, 63, 65, 91, 105, 117 (prime-factor map)
CODE_TOP_RADIX2 = 2  # fastecc_create_ex flag (A/B experiment): the top level of a power-of-two transform through the fused odd-radix kernel

WRITE_NONE = 0xFFFFFFFFFFFFFFFF  # entry of a device write list (update_batch_device, update_parity_batch_device): the row is skipped
READ_NONE = 0xFFFFFFFFFFFFFFFF  # entry of a device request list (read_batch_set_device, read_batch_device): row u of out is left alone
PATTERN_NONE = 0xFFFFFFFF  # pattern_of entry of the set calls (decode_batch_set, repair_batch_set, verify_batch_set, correct_batch_set): the stripe is neither read nor written

OK, E_INVAL, E_NOMEM, E_DEVICE, E_UNSUPPORTED, E_UNCORRECTABLE = 0, -1, -2, -3, -4, -5

_LIB = None


class FastEccError(RuntimeError):
    def __init__(self, code, what):
        self.code = code
        detail = lib().fastecc_last_error_detail().decode()
        super().__init__("%s: %s (%d)%s" % (what, lib().fastecc_strerror(code).decode(), code,
                                             " [" + detail + "]" if detail else ""))


def lib_path():
    # FASTECC_HIP_LIB lets experiments A/B another build of the same library (e.g. different hipcc flags)
    return os.environ.get("FASTECC_HIP_LIB") or _build.LIB_PATH


def lib():
    """Load libfastecc_hip.so (never falls back to anything else)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise FileNotFoundError(
            "%s not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(fastecc_amd has no CPU fallback)" % path)
    # One HIP runtime per process: PyTorch wheels bundle their own libamdhip64/libhsa-runtime64, and a
    # process that initialises two HSA runtimes loses the GPU in the second one ("no ROCm-capable
    # device").  Callers of this harness use torch for device memory, so let torch's runtime load first;
    # libfastecc_hip.so's DT_NEEDED libamdhip64.so.* then binds to the copy already in the process.  A
    # C++ host (fastecc_amd/host/rs_main.cpp) links the system runtime directly and has no such issue.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(path)
    vp, u64, u32, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
    L.fastecc_strerror.argtypes, L.fastecc_strerror.restype = [i32], ctypes.c_char_p
    L.fastecc_version.argtypes, L.fastecc_version.restype = [], i32
    L.fastecc_last_error_detail.argtypes, L.fastecc_last_error_detail.restype = [], ctypes.c_char_p
    L.fastecc_create.argtypes, L.fastecc_create.restype = [ctypes.POINTER(vp), u64, u64, u64, i32, i32], i32
    L.fastecc_create_ex.argtypes, L.fastecc_create_ex.restype = [ctypes.POINTER(vp), u64, u64, u64, i32, i32, ctypes.c_uint], i32
    L.fastecc_destroy.argtypes, L.fastecc_destroy.restype = [vp], None
    L.fastecc_encode.argtypes, L.fastecc_encode.restype = [vp, vp, vp, i32, vp], i32
    L.fastecc_encode_batch.argtypes, L.fastecc_encode_batch.restype = [vp, vp, vp, u64, vp], i32
    L.fastecc_encode_pool.argtypes, L.fastecc_encode_pool.restype = [vp, vp, vp, u64, vp], i32
    L.fastecc_encode_columns.argtypes, L.fastecc_encode_columns.restype = [vp, vp, vp, u64, u64, vp], i32
    L.fastecc_create_sharded.argtypes = [ctypes.POINTER(vp), u64, u64, u64, i32, ctypes.POINTER(i32), i32]
    L.fastecc_create_sharded.restype = i32
    L.fastecc_encode_sharded.argtypes, L.fastecc_encode_sharded.restype = [vp, ctypes.POINTER(vp), ctypes.POINTER(vp), vp, vp], i32
    L.fastecc_encode_sharded_blocks.argtypes = [vp, ctypes.POINTER(vp), i32, ctypes.POINTER(vp), vp]
    L.fastecc_encode_sharded_blocks.restype = i32
    L.fastecc_shard_info.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(u64), ctypes.POINTER(i32), i32]
    L.fastecc_shard_info.restype = i32
    L.fastecc_plan_describe.argtypes, L.fastecc_plan_describe.restype = [u64, u64, i32, ctypes.c_char_p, ctypes.c_size_t], i32
    L.fastecc_plan_twiddles.argtypes = [u64, u64, i32, i32, ctypes.POINTER(u32), ctypes.POINTER(ctypes.c_int32)]
    L.fastecc_plan_twiddles.restype = i32
    L.fastecc_encode_blocks.argtypes, L.fastecc_encode_blocks.restype = [vp, ctypes.POINTER(vp)], i32
    L.fastecc_ntt.argtypes, L.fastecc_ntt.restype = [vp, vp, i32, i32, vp], i32
    L.fastecc_scale_blocks.argtypes, L.fastecc_scale_blocks.restype = [vp, vp, u32, u32, i32, vp], i32
    L.fastecc_gf_binary.argtypes, L.fastecc_gf_binary.restype = [vp, i32, vp, vp, vp, u64, vp], i32
    L.fastecc_check_range.argtypes, L.fastecc_check_range.restype = [vp, vp, i32, vp, ctypes.POINTER(u64)], i32
    for name in ("mul", "pow"):
        f = getattr(L, "fastecc_gf_" + name)
        f.argtypes, f.restype = [u32, u32], u32
    for name in ("root", "inv"):
        f = getattr(L, "fastecc_gf_" + name)
        f.argtypes, f.restype = [u32], u32
    u8p = ctypes.POINTER(ctypes.c_uint8)
    L.fastecc_decode_prepare.argtypes, L.fastecc_decode_prepare.restype = [vp, u8p, u8p], i32
    L.fastecc_decode.argtypes, L.fastecc_decode.restype = [vp, vp, vp, i32, vp], i32
    L.fastecc_repair.argtypes, L.fastecc_repair.restype = [vp, vp, vp, i32, vp], i32
    L.fastecc_decode_batch.argtypes, L.fastecc_decode_batch.restype = [vp, vp, vp, u64, vp], i32
    L.fastecc_repair_batch.argtypes, L.fastecc_repair_batch.restype = [vp, vp, vp, u64, vp], i32
    L.fastecc_decode_prepare_set.argtypes, L.fastecc_decode_prepare_set.restype = [vp, u8p, u8p, u64], i32
    L.fastecc_decode_batch_set.argtypes, L.fastecc_decode_batch_set.restype = [vp, vp, vp, u64, ctypes.POINTER(u32), vp], i32
    L.fastecc_repair_batch_set.argtypes, L.fastecc_repair_batch_set.restype = [vp, vp, vp, u64, ctypes.POINTER(u32), vp], i32
    L.fastecc_read_batch_set.argtypes = [vp, vp, vp, u64, ctypes.POINTER(u32), ctypes.POINTER(u64), u64, u64, u64, vp, vp]
    L.fastecc_read_batch_set.restype = i32
    L.fastecc_read_batch.argtypes, L.fastecc_read_batch.restype = [vp, vp, vp, u64, ctypes.POINTER(u64), u64, u64, u64, vp, vp], i32
    L.fastecc_read_batch_set_device.argtypes, L.fastecc_read_batch_set_device.restype = [vp, vp, vp, u64, vp, vp, u64, u64, u64, vp, vp, vp], i32
    L.fastecc_read_batch_device.argtypes, L.fastecc_read_batch_device.restype = [vp, vp, vp, u64, vp, u64, u64, u64, vp, vp, vp], i32
    L.fastecc_scrub_erasures.argtypes, L.fastecc_scrub_erasures.restype = [vp, u8p, u8p], i32
    L.fastecc_verify.argtypes, L.fastecc_verify.restype = [vp, vp, vp, i32, vp, u64, ctypes.POINTER(i32)], i32
    for name in ("locate_errors", "correct"):
        f = getattr(L, "fastecc_" + name)
        f.argtypes, f.restype = [vp, vp, vp, i32, vp, u64, ctypes.POINTER(u64), u64, ctypes.POINTER(u64)], i32
    u64p = ctypes.POINTER(u64)
    for name in ("verify_batch", "correct_batch"):
        f = getattr(L, "fastecc_" + name)
        f.argtypes, f.restype = [vp, vp, vp, u64, vp, u64, u8p, u64p], i32
    L.fastecc_scrub_erasures_set.argtypes, L.fastecc_scrub_erasures_set.restype = [vp, u8p, u8p, u64], i32
    for name in ("verify_batch_set", "correct_batch_set"):
        f = getattr(L, "fastecc_" + name)
        f.argtypes, f.restype = [vp, vp, vp, u64, ctypes.POINTER(u32), vp, u64, u8p, u64p], i32
    L.fastecc_locate_errors_batch.argtypes = [vp, vp, vp, u64, vp, u64, u8p, u64p, u64, ctypes.POINTER(u32), u64p]
    L.fastecc_locate_errors_batch.restype = i32
    L.fastecc_locate_errors_batch_set.argtypes = [vp, vp, vp, u64, ctypes.POINTER(u32), vp, u64, u8p, u64p, u64, ctypes.POINTER(u32), u64p]
    L.fastecc_locate_errors_batch_set.restype = i32
    L.fastecc_scrub_fingerprints.argtypes, L.fastecc_scrub_fingerprints.restype = [vp, vp, vp, u64, u64p, i32, vp, u64, ctypes.POINTER(u32), u8p], i32
    L.fastecc_update.argtypes, L.fastecc_update.restype = [vp, vp, vp, u64p, u64, vp, i32, vp], i32
    L.fastecc_update_parity.argtypes, L.fastecc_update_parity.restype = [vp, vp, u64p, u64, vp, vp, i32, vp], i32
    L.fastecc_update_batch.argtypes, L.fastecc_update_batch.restype = [vp, vp, vp, u64, u64p, u64, vp, vp], i32
    L.fastecc_update_parity_batch.argtypes, L.fastecc_update_parity_batch.restype = [vp, vp, u64, u64p, u64, vp, vp, vp], i32
    L.fastecc_update_batch_set.argtypes, L.fastecc_update_batch_set.restype = [vp, vp, vp, u64, ctypes.POINTER(u32), u64p, u64, vp, vp], i32
    L.fastecc_update_parity_batch_set.argtypes = [vp, vp, u64, ctypes.POINTER(u32), u64p, u64, vp, vp, vp]
    L.fastecc_update_parity_batch_set.restype = i32
    L.fastecc_update_batch_window.argtypes, L.fastecc_update_batch_window.restype = [vp, vp, vp, u64, u64p, u64, u64, u64, vp, vp], i32
    L.fastecc_update_parity_batch_window.argtypes = [vp, vp, u64, u64p, u64, u64, u64, vp, vp, vp]
    L.fastecc_update_parity_batch_window.restype = i32
    L.fastecc_update_batch_set_window.argtypes = [vp, vp, vp, u64, ctypes.POINTER(u32), u64p, u64, u64, u64, vp, vp]
    L.fastecc_update_batch_set_window.restype = i32
    L.fastecc_update_parity_batch_set_window.argtypes = [vp, vp, u64, ctypes.POINTER(u32), u64p, u64, u64, u64, vp, vp, vp]
    L.fastecc_update_parity_batch_set_window.restype = i32
    L.fastecc_update_batch_device.argtypes = [vp, vp, vp, u64, vp, u64, u32, u64, u64, vp, vp, vp]
    L.fastecc_update_batch_device.restype = i32
    L.fastecc_update_parity_batch_device.argtypes = [vp, vp, u64, vp, u64, u32, u64, u64, vp, vp, vp, vp]
    L.fastecc_update_parity_batch_device.restype = i32
    L.fastecc_update_batch_set_device.argtypes = [vp, vp, vp, u64, vp, vp, u64, u32, u64, u64, u64, vp, vp, vp]
    L.fastecc_update_batch_set_device.restype = i32
    L.fastecc_update_parity_batch_set_device.argtypes = [vp, vp, u64, vp, vp, u64, u32, u64, u64, vp, vp, vp, vp]
    L.fastecc_update_parity_batch_set_device.restype = i32
    L.fastecc_code_coefficient.argtypes = [u64, u64, ctypes.c_uint, u64, u64, ctypes.POINTER(u32)]
    L.fastecc_code_coefficient.restype = i32
    L.fastecc_gf_berlekamp_massey.argtypes = [ctypes.POINTER(u32), u32, ctypes.POINTER(u32), u32]
    L.fastecc_gf_berlekamp_massey.restype = i32
    L.fastecc_pack_blocks.argtypes, L.fastecc_pack_blocks.restype = [vp, vp, vp, i32, vp], i32
    L.fastecc_unpack_blocks.argtypes, L.fastecc_unpack_blocks.restype = [vp, vp, vp, i32, vp, ctypes.POINTER(u64)], i32
    pair = ctypes.POINTER(u64)
    L.fastecc_gf61_mul.argtypes, L.fastecc_gf61_mul.restype = [pair, pair, pair], i32
    L.fastecc_gf61_pow.argtypes, L.fastecc_gf61_pow.restype = [pair, u64, pair], i32
    L.fastecc_gf61_inv.argtypes, L.fastecc_gf61_inv.restype = [pair, pair], i32
    L.fastecc_gf61_root.argtypes, L.fastecc_gf61_root.restype = [u64, pair], i32
    L.fastecc_gf61_binary.argtypes, L.fastecc_gf61_binary.restype = [vp, i32, vp, vp, vp, u64, vp], i32
    L.fastecc_gf61_update.argtypes, L.fastecc_gf61_update.restype = [vp, vp, vp, u64p, u64, vp, vp], i32
    L.fastecc_gf61_update_parity.argtypes, L.fastecc_gf61_update_parity.restype = [vp, vp, u64p, u64, vp, vp, vp], i32
    L.fastecc_gf61_code_coefficient.argtypes, L.fastecc_gf61_code_coefficient.restype = [u64, u64, u64, u64, pair], i32
    L.fastecc_profile_enable.argtypes, L.fastecc_profile_enable.restype = [vp, i32], i32
    L.fastecc_profile_reset.argtypes, L.fastecc_profile_reset.restype = [vp], i32
    L.fastecc_profile_read.argtypes = [vp, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_double),
                                       ctypes.POINTER(u64), i32]
    L.fastecc_profile_read.restype = i32
    L.fastecc_profile_read_bytes.argtypes = [vp, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_double),
                                             ctypes.POINTER(u64), ctypes.POINTER(u64), i32]
    L.fastecc_profile_read_bytes.restype = i32
    L.fastecc_set_option.argtypes, L.fastecc_set_option.restype = [vp, ctypes.c_char_p, i32], i32
    L.fastecc_plan_string.argtypes, L.fastecc_plan_string.restype = [vp], ctypes.c_char_p
    L.fastecc_set_plan.argtypes, L.fastecc_set_plan.restype = [vp, i32], i32
    _LIB = L
    return L


def _check(code, what):
    if code < 0:
        raise FastEccError(code, what)
    return code


def _addr(x):
    """Integer address of a torch tensor / numpy array / int."""
    if x is None:
        return None
    if isinstance(x, int):
        return x
    if hasattr(x, "data_ptr"):
        return x.data_ptr()
    if hasattr(x, "ctypes"):
        return x.ctypes.data
    raise TypeError("need an address, torch tensor or numpy array")


class Encoder:
    """(n,k) Reed-Solomon encoder: the RS.cpp:22-68 operation behind the C ABI (include/fastecc.h).

    ``data`` is a device tensor (or raw address) of k*block_bytes bytes laid out block-major, exactly the
    ``T** data`` stripe of RS.cpp:28-33 stored back to back; ``parity`` holds n-k blocks the same way.
    (n,k) = (2N,N), N = 2^m, is the reference's configuration (parity block j = f(w_2N^(2j+1))); fastecc_create
    also accepts n-k = k/2 .. k/16 (a sub-coset of that parity), n = 4k / 8k (further cosets) and any other
    (n,k) with n-k <= 2^ceil(log2 k) by zero extension, all over GF(0xFFF00001) with 4-byte words; and
    (2N,N) over GF((2^61-1)^2) with 16-byte elements (``field=FIELD_GF_P61_SQUARED``).
    """

    def __init__(self, n, k, block_bytes, device=0, field=FIELD_GF_FFF00001, flags=0):
        self._h = ctypes.c_void_p()
        self.n, self.k, self.block_bytes, self.device, self.field = n, k, block_bytes, device, field
        if flags:
            _check(lib().fastecc_create_ex(ctypes.byref(self._h), n, k, block_bytes, field, device, flags), "fastecc_create_ex")
        else:
            _check(lib().fastecc_create(ctypes.byref(self._h), n, k, block_bytes, field, device), "fastecc_create")

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            lib().fastecc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def parity_blocks(self):
        return self.n - self.k

    @property
    def words_per_block(self):
        return self.block_bytes // 4

    def encode(self, data, parity=None, stream=0, mem=MEM_DEVICE):
        """parity <- encode(data); parity=None encodes in place (the reference's behaviour)."""
        if parity is None:
            parity = data
        _check(lib().fastecc_encode(self._h, _addr(data), _addr(parity), mem, stream or None), "fastecc_encode")
        return parity

    def encode_columns(self, data, parity, col0_words, width_words, stream=0):
        """Encode only words [col0, col0+width) of every block (columns are independent transforms)."""
        _check(lib().fastecc_encode_columns(self._h, _addr(data), _addr(parity), col0_words, width_words, stream or None),
               "fastecc_encode_columns")
        return parity

    def encode_batch(self, data, parity, count, stream=0):
        """`count` stripes stored back to back in device memory, one launch per pass."""
        if parity is None:
            parity = data
        _check(lib().fastecc_encode_batch(self._h, _addr(data), _addr(parity), count, stream or None), "fastecc_encode_batch")
        return parity

    def encode_pool(self, data, parity, count, stream=0):
        """Write a pool: `count` stripes back to back in device memory (the layout of decode_batch: stripe b's k data blocks at
        data + b*k*block_bytes, its n - k parity blocks at parity + b*(n-k)*block_bytes); every stripe's parity is what encode gives for
        it alone.  Any GF(0xFFF00001) code; data is read only and must not overlap parity.  Option "encode_pool_kernel" picks the kernel."""
        count = self._batch_count(count)
        _check(lib().fastecc_encode_pool(self._h, _addr(data), _addr(parity), count, stream or None), "fastecc_encode_pool")
        return parity

    def encode_host(self, data_np, parity_np=None):
        return self.encode(data_np, parity_np, mem=MEM_HOST)

    def encode_blocks(self, block_addresses):
        arr = (ctypes.c_void_p * len(block_addresses))(*block_addresses)
        _check(lib().fastecc_encode_blocks(self._h, arr), "fastecc_encode_blocks")

    def ntt(self, data, inverse=False, stream=0, mem=MEM_DEVICE):
        _check(lib().fastecc_ntt(self._h, _addr(data), int(inverse), mem, stream or None), "fastecc_ntt")
        return data

    def scale_blocks(self, data, scale, base, stream=0, mem=MEM_DEVICE):
        _check(lib().fastecc_scale_blocks(self._h, _addr(data), scale, base, mem, stream or None),
               "fastecc_scale_blocks")
        return data

    def gf_binary(self, op, x, y, out, count, stream=0):
        code = {"add": 0, "sub": 1, "mul": 2, "mul_mont": 3}[op] if isinstance(op, str) else op
        _check(lib().fastecc_gf_binary(self._h, code, _addr(x), _addr(y), _addr(out), count, stream or None),
               "fastecc_gf_binary")
        return out

    # op codes of fastecc_gf61_binary (include/fastecc.h: FASTECC_GF61_OP_*); the run ops take "run_dif" / "run_dif_inv" / "run_dit" + levels
    GF61_OPS = {"add": 0, "sub": 1, "mul": 2, "mul_raw": 3, "mul_w8": 4, "mul_w8i": 5, "mul_w8_inv": 6, "mul_w8i_inv": 7, "fold": 8, "canon": 9,
                "run_dif": 16, "run_dif_inv": 20, "run_dit": 24}

    def gf61_binary(self, op, x, y, out, count, stream=0, levels=1):
        """The 64-bit field's device arithmetic on `count` elements (re, im) of device memory, results NOT made canonical (tests only).
        op: a name of GF61_OPS (run ops: `levels` = 1..4 radix-2 levels on runs of 2^levels elements) or a raw op code."""
        if isinstance(op, str):
            code = self.GF61_OPS[op]
            if op.startswith("run_"):
                if not 1 <= levels <= 4:
                    raise ValueError("a run has 1..4 levels")
                code += levels - 1
        else:
            code = op
        _check(lib().fastecc_gf61_binary(self._h, code, _addr(x), _addr(y), _addr(out), count, stream or None), "fastecc_gf61_binary")
        return out

    def check_range(self, data, stream=0, mem=MEM_DEVICE):
        """Number of words >= p in the stripe (0 = encodable); README.md:160-162 of the reference."""
        bad = ctypes.c_uint64()
        _check(lib().fastecc_check_range(self._h, _addr(data), mem, stream or None, ctypes.byref(bad)), "fastecc_check_range")
        return int(bad.value)

    def decode_prepare(self, data_present, parity_present):
        """Erasure pattern: k data flags and n - k parity flags (truthy = the block survives)."""
        if len(data_present) != self.k or len(parity_present) != self.n - self.k:
            raise ValueError("need k data flags and n - k parity flags")
        keep_d, dp = self._flags(data_present, self.k)
        keep_p, pp = self._flags(parity_present, self.n - self.k)
        _check(lib().fastecc_decode_prepare(self._h, dp, pp), "fastecc_decode_prepare")
        del keep_d, keep_p

    @staticmethod
    def _flags(v, count):
        """(object to keep alive, uint8 pointer) of `count` presence flags; None stays a null pointer."""
        if v is None:
            return None, None
        # a contiguous uint8 numpy array goes through as it is (the C ABI takes plain byte arrays); anything else is converted
        if hasattr(v, "ctypes") and getattr(v, "dtype", None) is not None and v.dtype.itemsize == 1 and v.flags["C_CONTIGUOUS"]:
            return v, ctypes.cast(v.ctypes.data, ctypes.POINTER(ctypes.c_uint8))
        arr = (ctypes.c_uint8 * count)(*[1 if x else 0 for x in v])
        return arr, arr

    def decode(self, data, parity, stream=0, mem=MEM_DEVICE):
        """Recover the erased data blocks in place (README.md:102-119); parity is read only."""
        _check(lib().fastecc_decode(self._h, _addr(data), _addr(parity), mem, stream or None), "fastecc_decode")
        return data

    def repair(self, data, parity, stream=0, mem=MEM_DEVICE):
        """decode, then rebuild the erased parity blocks as well (both buffers are written where blocks were lost)."""
        _check(lib().fastecc_repair(self._h, _addr(data), _addr(parity), mem, stream or None), "fastecc_repair")
        return data, parity

    @staticmethod
    def _batch_count(count):
        if isinstance(count, bool) or not isinstance(count, int):
            raise TypeError("count must be an int")
        if count < 1 or count >= 1 << 64:
            raise ValueError("count must be in [1, 2^64)")
        return count

    def decode_batch(self, data, parity, count, stream=0):
        """`count` stripes back to back in device memory, all with the prepared erasure pattern: decode of each (parity is read only)."""
        count = self._batch_count(count)
        _check(lib().fastecc_decode_batch(self._h, _addr(data), _addr(parity), count, stream or None), "fastecc_decode_batch")
        return data

    def repair_batch(self, data, parity, count, stream=0):
        """repair of `count` stripes back to back in device memory, all with the prepared erasure pattern."""
        count = self._batch_count(count)
        _check(lib().fastecc_repair_batch(self._h, _addr(data), _addr(parity), count, stream or None), "fastecc_repair_batch")
        return data, parity

    def decode_prepare_set(self, data_present, parity_present):
        """A set of P erasure patterns for decode_batch_set / repair_batch_set: P rows of k data flags and P rows of n - k parity flags
        (truthy = the block survives); every pattern loses at most 16 blocks and keeps at least k.  P = 0 (two empty arguments) clears the
        set.  Independent of the decode_prepare pattern."""
        self._pattern_set(lib().fastecc_decode_prepare_set, "fastecc_decode_prepare_set", data_present, parity_present)

    def _pattern_set(self, fn, what, data_present, parity_present):
        """fn(handle, P x k data flags, P x (n - k) parity flags, P) with the shapes checked first"""
        import numpy as np
        P = len(data_present)
        if len(parity_present) != P:
            raise ValueError("need as many rows of parity flags as of data flags")
        m = self.n - self.k
        if P and (any(len(r) != self.k for r in data_present) or any(len(r) != m for r in parity_present)):
            raise ValueError("need P x k data flags and P x (n - k) parity flags")

        def flat(v, width):
            # a contiguous uint8 numpy array goes through as it is; anything else is converted
            if isinstance(v, np.ndarray) and v.dtype.itemsize == 1 and v.flags["C_CONTIGUOUS"]:
                return v
            return np.ascontiguousarray(np.asarray(v, dtype=bool).reshape(P, width), dtype=np.uint8)
        u8p = ctypes.POINTER(ctypes.c_uint8)
        dp, pp = (flat(data_present, self.k), flat(parity_present, m)) if P else (None, None)
        _check(fn(self._h, dp.ctypes.data_as(u8p) if P else None, pp.ctypes.data_as(u8p) if P else None, P), what)

    @staticmethod
    def _pattern_list(pattern_of, count):
        """(object to keep alive, uint32 pointer) of the `count` pattern indices of a set call"""
        import numpy as np
        if len(pattern_of) != count:
            raise ValueError("pattern_of needs one entry per stripe")
        if isinstance(pattern_of, np.ndarray) and pattern_of.dtype == np.uint32 and pattern_of.flags["C_CONTIGUOUS"]:
            arr = pattern_of
        else:
            idx = [int(q) for q in pattern_of]
            if any(q < 0 or q > PATTERN_NONE for q in idx):
                raise ValueError("a pattern index is a uint32")
            arr = np.array(idx, dtype=np.uint32)
        return arr, arr.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))

    def decode_batch_set(self, data, parity, count, pattern_of, stream=0):
        """`count` stripes back to back in device memory, stripe b with pattern pattern_of[b] of the prepared set (PATTERN_NONE: the stripe
        is not touched): decode of each (parity is read only)."""
        count = self._batch_count(count)
        keep, po = self._pattern_list(pattern_of, count)
        _check(lib().fastecc_decode_batch_set(self._h, _addr(data), _addr(parity), count, po, stream or None), "fastecc_decode_batch_set")
        del keep
        return data

    def repair_batch_set(self, data, parity, count, pattern_of, stream=0):
        """repair of `count` stripes back to back in device memory, stripe b with pattern pattern_of[b] of the prepared set."""
        count = self._batch_count(count)
        keep, po = self._pattern_list(pattern_of, count)
        _check(lib().fastecc_repair_batch_set(self._h, _addr(data), _addr(parity), count, po, stream or None), "fastecc_repair_batch_set")
        del keep
        return data, parity

    @classmethod
    def _read_list(cls, reads):
        """(entries, object to keep alive, uint64 pointer) of the pool block indices of a read call"""
        import numpy as np
        if isinstance(reads, np.ndarray) and reads.dtype == np.uint64 and reads.ndim == 1 and reads.flags["C_CONTIGUOUS"]:
            return len(reads), reads, reads.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))  # goes through as it is
        idx = [int(b) for b in reads]
        if any(b < 0 or b >= 1 << 64 for b in idx):
            raise ValueError("a pool block index is a uint64")
        n, arr = cls._block_list(idx)
        return n, arr, arr

    def _read_window(self, col0, width):
        if isinstance(col0, bool) or not isinstance(col0, int) or (width is not None and (isinstance(width, bool) or not isinstance(width, int))):
            raise TypeError("col0 and width are ints (words)")
        if col0 < 0 or col0 >= 1 << 64:
            raise ValueError("col0 must be in [0, 2^64)")
        if width is None:
            width = self.words_per_block - col0  # the whole block from col0 on
        if width < 1 or width >= 1 << 64:
            raise ValueError("the window must hold at least one word of the block")
        return col0, width

    def read_batch_set(self, data, parity, count, pattern_of, reads, out, col0=0, width=None, stream=0):
        """Degraded reads of a pool of `count` stripes (the layout of decode_batch) with stripe b under pattern pattern_of[b] of the
        decode_prepare_set set (PATTERN_NONE: every block present): row u of `out` (width words each, device memory) receives the words
        [col0, col0 + width) of pool block reads[u] = b * k + i — a copy where the block is present, else what decode would rebuild.  The pool
        is not written.  width=None: the whole block from col0 on.  Any order, duplicates allowed."""
        count = self._batch_count(count)
        keep, po = self._pattern_list(pattern_of, count)
        col0, width = self._read_window(col0, width)
        n, keep_r, arr = self._read_list(reads)
        _check(lib().fastecc_read_batch_set(self._h, _addr(data), _addr(parity), count, po, arr, n, col0, width, _addr(out), stream or None),
               "fastecc_read_batch_set")
        del keep, keep_r
        return out

    def read_batch(self, data, parity, count, reads, out, col0=0, width=None, stream=0):
        """read_batch_set with every stripe under the single decode_prepare pattern (direct-path patterns only)."""
        count = self._batch_count(count)
        col0, width = self._read_window(col0, width)
        n, keep_r, arr = self._read_list(reads)
        _check(lib().fastecc_read_batch(self._h, _addr(data), _addr(parity), count, arr, n, col0, width, _addr(out), stream or None), "fastecc_read_batch")
        del keep_r
        return out

    def _device_reads(self, count, n_reads, col0, width):
        """the checked (count, n_reads, col0, width) of a device-list read; count and the window as _device_list checks them"""
        count = self._batch_count(count)
        if isinstance(n_reads, bool) or not isinstance(n_reads, int):
            raise TypeError("n_reads must be an int")
        if n_reads < 0 or n_reads >= 1 << 64:
            raise ValueError("n_reads must be in [0, 2^64)")
        col0, width = self._read_window(col0, width)
        return count, n_reads, col0, width

    def read_batch_set_device(self, data, parity, count, pattern_of, reads, n_reads, out, status, col0=0, width=None, stream=0):
        """read_batch_set with the request list and pattern_of in DEVICE memory: `reads` (a device tensor or address, uint64 entries, 8-byte
        aligned) holds n_reads entries b * k + i or READ_NONE (row u of `out` is left alone), `pattern_of` (uint32, `count` entries) the
        pattern of every stripe; both are read when the call's kernels run on `stream`, never by the host.  `status` (one uint64 of device
        memory) is set by the call on the stream: 0 when every request was served, else (error code as uint32) << 32 | one row at fault, and
        then no word of `out` has been written.  col0, width (words; width=None: from col0 to the end of the block) as for read_batch_set."""
        count, n_reads, col0, width = self._device_reads(count, n_reads, col0, width)
        _check(lib().fastecc_read_batch_set_device(self._h, _addr(data), _addr(parity), count, _addr(pattern_of), _addr(reads), n_reads, col0, width,
                                                   _addr(out), _addr(status), stream or None), "fastecc_read_batch_set_device")
        return out

    def read_batch_device(self, data, parity, count, reads, n_reads, out, status, col0=0, width=None, stream=0):
        """read_batch_set_device with every stripe under the single decode_prepare pattern (direct-path patterns only)."""
        count, n_reads, col0, width = self._device_reads(count, n_reads, col0, width)
        _check(lib().fastecc_read_batch_device(self._h, _addr(data), _addr(parity), count, _addr(reads), n_reads, col0, width, _addr(out),
                                               _addr(status), stream or None), "fastecc_read_batch_device")
        return out

    def scrub_erasures(self, data_present=None, parity_present=None):
        """Name the blocks that are known to be absent (a device is down) for verify, locate_errors, correct and their batched forms:
        k data flags and n - k parity flags, truthy = present, None = every block of that part is present; both None clears the
        pattern.  Absent blocks are never read; correct rebuilds them together with the blocks it locates.  Independent of the
        decode_prepare pattern."""
        if data_present is not None and len(data_present) != self.k:
            raise ValueError("need k data flags")
        if parity_present is not None and len(parity_present) != self.n - self.k:
            raise ValueError("need n - k parity flags")
        keep_d, dp = self._flags(data_present, self.k)
        keep_p, pp = self._flags(parity_present, self.n - self.k)
        _check(lib().fastecc_scrub_erasures(self._h, dp, pp), "fastecc_scrub_erasures")
        del keep_d, keep_p

    def verify(self, data, parity, seed=0, stream=0, mem=MEM_DEVICE):
        """True iff every word of every present block is < p and the present blocks of the k data + n - k parity blocks agree with a
        codeword (fingerprints drawn from `seed`; every block is present unless scrub_erasures named some absent)."""
        ok = ctypes.c_int()
        _check(lib().fastecc_verify(self._h, _addr(data), _addr(parity), mem, stream or None, seed, ctypes.byref(ok)), "fastecc_verify")
        return bool(ok.value)

    def _pool_patterns(self, pattern_of, count):
        """(object to keep alive, the arguments a pool call's set form takes after `count`): none for the single-pattern form (pattern_of None)"""
        if pattern_of is None:
            return None, ()
        keep, po = self._pattern_list(pattern_of, count)
        return keep, (po,)

    def _scrub_batch(self, fn, data, parity, count, seed, stream, pattern_of=None):
        """(return code, uint8 array with one entry per stripe) of a batched verify or correct, in its set form where pattern_of is given"""
        import numpy as np
        count = self._batch_count(count)
        keep, po = self._pool_patterns(pattern_of, count)
        out = np.zeros(count, np.uint8)
        bad = ctypes.c_uint64()
        code = fn(self._h, _addr(data), _addr(parity), count, *po, stream or None, seed, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), ctypes.byref(bad))
        del keep
        return code, out

    @staticmethod
    def _corrected(code, what, status):
        """the status array of a batched correction, or its error (E_UNCORRECTABLE carries the array)"""
        if code == E_UNCORRECTABLE:
            err = FastEccError(code, what)
            err.status = status
            raise err
        _check(code, what)
        return status

    def _locate_batch(self, fn, what, data, parity, count, seed, stream, pattern_of=None):
        """(status, lists) of a batched location call, in its set form where pattern_of is given, or its error (E_UNCORRECTABLE carries both)"""
        import numpy as np
        count = self._batch_count(count)
        keep, po = self._pool_patterns(pattern_of, count)
        cap = self.n - self.k
        status = np.zeros(count, np.uint8)
        blocks = np.zeros(count * cap, np.uint64)
        counts = np.zeros(count, np.uint32)
        bad = ctypes.c_uint64()
        code = fn(self._h, _addr(data), _addr(parity), count, *po, stream or None, seed, status.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                  blocks.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), cap, counts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), ctypes.byref(bad))
        del keep
        lists = [[int(x) for x in blocks[b * cap:b * cap + min(int(counts[b]), cap)]] for b in range(count)] if code in (OK, E_UNCORRECTABLE) else None
        if code == E_UNCORRECTABLE:
            err = FastEccError(code, what)
            err.status, err.lists = status, lists
            raise err
        _check(code, what)
        return status, lists

    def verify_batch(self, data, parity, count, seed=0, stream=0):
        """`count` stripes back to back in device memory (the layout of decode_batch): a numpy bool array, True where verify with the
        same seed finds the stripe consistent.  Reads only."""
        code, out = self._scrub_batch(lib().fastecc_verify_batch, data, parity, count, seed, stream)
        _check(code, "fastecc_verify_batch")
        return out.astype(bool)

    def correct_batch(self, data, parity, count, seed=0, stream=0):
        """verify_batch, then what correct does to each inconsistent stripe (replaces the prepared erasure pattern; which pattern is
        left behind is unspecified).  Option "correct_batch_mode": 2 = correct stripe by stripe, 1 = one batched location pass and one
        repair per distinct set of lost blocks, 0 (default) = 1 from two qualifying stripes on; the same status and bytes in every mode.
        Returns the numpy uint8 status array: 0 = consistent and untouched, 1 = corrected, 2 = uncorrectable.  If any stripe is
        uncorrectable, raises FastEccError with code E_UNCORRECTABLE after the others were corrected; the full status array is its
        `status` attribute."""
        code, out = self._scrub_batch(lib().fastecc_correct_batch, data, parity, count, seed, stream)
        return self._corrected(code, "fastecc_correct_batch", out)

    def scrub_erasures_set(self, data_present, parity_present):
        """A set of P absent-block patterns for verify_batch_set / correct_batch_set (a degraded pool with rotated placement): P rows of k
        data flags and P rows of n - k parity flags (truthy = present), the arrays decode_prepare_set takes; a pattern names 0 .. n - k
        blocks absent.  P = 0 (two empty arguments) clears the set.  Independent of the scrub_erasures pattern and of both decode patterns."""
        self._pattern_set(lib().fastecc_scrub_erasures_set, "fastecc_scrub_erasures_set", data_present, parity_present)

    def verify_batch_set(self, data, parity, count, pattern_of, seed=0, stream=0):
        """verify_batch with stripe b under pattern pattern_of[b] of the scrub_erasures_set set: a numpy bool array, True where
        scrub_erasures(that pattern) + verify with the same seed finds the stripe consistent, and for PATTERN_NONE stripes, which are
        not read.  Reads only."""
        code, out = self._scrub_batch(lib().fastecc_verify_batch_set, data, parity, count, seed, stream, pattern_of)
        _check(code, "fastecc_verify_batch_set")
        return out.astype(bool)

    def correct_batch_set(self, data, parity, count, pattern_of, seed=0, stream=0):
        """verify_batch_set, then what scrub_erasures(its pattern) + correct does to each inconsistent stripe (replaces the prepared
        erasure pattern — which one is left behind is unspecified — not the decode_prepare_set set).  Option "correct_batch_mode": 2 = stripe
        by stripe, 1 = one batched location pass and one grouped repair through a pattern set private to the call, 0 (default) = 1 from two
        qualifying stripes on; the same status and bytes in every mode.  Returns the numpy uint8 status array: 0 = consistent or skipped and untouched,
        1 = corrected (the whole codeword is back), 2 = uncorrectable.  If any stripe is uncorrectable, raises FastEccError with code
        E_UNCORRECTABLE after the others were corrected; the full status array is its `status` attribute."""
        code, out = self._scrub_batch(lib().fastecc_correct_batch_set, data, parity, count, seed, stream, pattern_of)
        return self._corrected(code, "fastecc_correct_batch_set", out)

    def locate_errors_batch(self, data, parity, count, seed=0, stream=0):
        """locate_errors for each of `count` stripes back to back in device memory: (status, lists) with the numpy uint8 status array
        (0 = consistent, 1 = located, 2 = cannot be located) and one list of codeword indices per stripe (increasing; [] for status 0
        and 2).  Reads only.  If any stripe cannot be located, raises FastEccError with code E_UNCORRECTABLE carrying both as its
        `status` and `lists` attributes."""
        return self._locate_batch(lib().fastecc_locate_errors_batch, "fastecc_locate_errors_batch", data, parity, count, seed, stream)

    def locate_errors_batch_set(self, data, parity, count, pattern_of, seed=0, stream=0):
        """locate_errors_batch with stripe b under pattern pattern_of[b] of the scrub_erasures_set set: (status, lists) as there, each stripe's
        answer the one scrub_erasures(that pattern) + locate_errors with the same seed gives; absent blocks are neither read nor listed, and a
        PATTERN_NONE stripe is not read and has status 0.  Reads only.  Raises like locate_errors_batch, with `status` and `lists`."""
        return self._locate_batch(lib().fastecc_locate_errors_batch_set, "fastecc_locate_errors_batch_set", data, parity, count, seed, stream, pattern_of)

    def scrub_fingerprints(self, data, parity, count=1, form=0, stripes=None, seed=0, stream=0):
        """What the fingerprint pass of the scrub calls computes (tests only): (F, big) with F a numpy uint32 array [entries, n, 3], F[i, j, c]
        = sum_w rho_c[w] * word w of block j of entry i mod p, and big a bool array, True where a block of the entry holds a word >= p.
        form 0: the single-stripe pass (count 1); 1: the batch pass over `count` stripes; 2: the list pass over the stripes `stripes` of the pool."""
        import numpy as np
        arr = None
        if stripes is not None:
            count, arr = self._block_list(stripes)
        out = np.zeros((count, self.n, 3), np.uint32)
        big = np.zeros(count, np.uint8)
        _check(lib().fastecc_scrub_fingerprints(self._h, _addr(data), _addr(parity), count, arr, form, stream or None, seed,
                                                out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), big.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))),
               "fastecc_scrub_fingerprints")
        return out, big.astype(bool)

    def _located(self, fn, what, data, parity, seed, stream, mem):
        cap = self.n - self.k
        out = (ctypes.c_uint64 * max(cap, 1))()
        count = ctypes.c_uint64()
        _check(fn(self._h, _addr(data), _addr(parity), mem, stream or None, seed, out, cap, ctypes.byref(count)), what)
        return [int(out[i]) for i in range(min(int(count.value), cap))]

    def locate_errors(self, data, parity, seed=0, stream=0, mem=MEM_DEVICE):
        """Codeword indices (data i -> i, parity j -> k + j) of the corrupted blocks, increasing; [] if consistent.  Reads only.
        Raises FastEccError with code E_UNCORRECTABLE when they cannot be located."""
        return self._located(lib().fastecc_locate_errors, "fastecc_locate_errors", data, parity, seed, stream, mem)

    def correct(self, data, parity, seed=0, stream=0, mem=MEM_DEVICE):
        """locate_errors, then rebuild those blocks in place (replaces the prepared erasure pattern); returns the located blocks."""
        return self._located(lib().fastecc_correct, "fastecc_correct", data, parity, seed, stream, mem)

    @staticmethod
    def _block_list(blocks):
        """(entries, uint64 pointer or array) of a list of block or stripe indices"""
        import numpy as np
        if isinstance(blocks, np.ndarray) and blocks.dtype == np.uint64 and blocks.ndim == 1 and blocks.flags["C_CONTIGUOUS"] and len(blocks):
            return len(blocks), blocks.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))  # goes through as it is (the pointer keeps the array alive)
        idx = [int(b) for b in blocks]
        return len(idx), (ctypes.c_uint64 * max(len(idx), 1))(*idx)

    def update(self, data, parity, blocks, new, stream=0, mem=MEM_DEVICE):
        """Small write: data blocks `blocks` become the len(blocks) contiguous blocks of `new`; the parity is brought up to date
        from the change alone (the rest of the stripe is not read).  data and parity then equal encode of the new stripe."""
        count, arr = self._block_list(blocks)
        _check(lib().fastecc_update(self._h, _addr(data), _addr(parity), arr, count, _addr(new), mem, stream or None), "fastecc_update")
        return data, parity

    def update_parity(self, parity, blocks, new, old=None, stream=0, mem=MEM_DEVICE):
        """parity += the effect of data blocks `blocks` changing from `old` to `new` (contiguous blocks each; old=None: from zero)."""
        count, arr = self._block_list(blocks)
        _check(lib().fastecc_update_parity(self._h, _addr(parity), arr, count, _addr(old), _addr(new), mem, stream or None),
               "fastecc_update_parity")
        return parity

    def gf61_update(self, data, parity, blocks, new, stream=0):
        """update() for a FIELD_GF_P61_SQUARED context (16-byte elements, device memory): data blocks `blocks` become the len(blocks)
        contiguous blocks of `new` and the parity follows; data and parity then equal encode of the new stripe."""
        count, arr = self._block_list(blocks)
        _check(lib().fastecc_gf61_update(self._h, _addr(data), _addr(parity), arr, count, _addr(new), stream or None), "fastecc_gf61_update")
        return data, parity

    def gf61_update_parity(self, parity, blocks, new, old=None, stream=0):
        """update_parity() for a FIELD_GF_P61_SQUARED context: parity += the effect of data blocks `blocks` changing from `old` to `new`
        (contiguous blocks each; old=None: from zero)."""
        count, arr = self._block_list(blocks)
        _check(lib().fastecc_gf61_update_parity(self._h, _addr(parity), arr, count, _addr(old), _addr(new), stream or None),
               "fastecc_gf61_update_parity")
        return parity

    def _write_window(self, col0, width):
        """None for the whole block (col0=0, width=None: the whole-block entry point), else the checked (col0, width) of a window call"""
        if width is None and isinstance(col0, int) and not isinstance(col0, bool) and col0 == 0:
            return None
        return self._read_window(col0, width)

    def update_batch(self, data, parity, count, writes, new, stream=0, col0=0, width=None):
        """Small writes into a pool of `count` stripes back to back in device memory (the layout of decode_batch): pool block
        writes[u] = b * k + i (data block i of stripe b; distinct, any order) becomes row u of `new`, and every touched stripe's parity is
        brought up to date — data and parity of those stripes then equal encode of the new stripe.  Other stripes are not touched.
        A window (col0, width in words; width=None: from col0 to the end of the block): row u of `new` holds `width` words and replaces the
        words [col0, col0 + width) of its block; no word outside those columns is read or written, in any block."""
        count = self._batch_count(count)
        window = self._write_window(col0, width)
        n, arr = self._block_list(writes)
        if window is None:
            _check(lib().fastecc_update_batch(self._h, _addr(data), _addr(parity), count, arr, n, _addr(new), stream or None), "fastecc_update_batch")
        else:
            _check(lib().fastecc_update_batch_window(self._h, _addr(data), _addr(parity), count, arr, n, window[0], window[1], _addr(new), stream or None),
                   "fastecc_update_batch_window")
        return data, parity

    def update_parity_batch(self, parity, count, writes, new, old=None, stream=0, col0=0, width=None):
        """update_batch for the parity alone: pool blocks `writes` changed from row u of `old` (None: from zero) to row u of `new` (a window: rows
        of `width` words, as for update_batch)."""
        count = self._batch_count(count)
        window = self._write_window(col0, width)
        n, arr = self._block_list(writes)
        if window is None:
            _check(lib().fastecc_update_parity_batch(self._h, _addr(parity), count, arr, n, _addr(old), _addr(new), stream or None),
                   "fastecc_update_parity_batch")
        else:
            _check(lib().fastecc_update_parity_batch_window(self._h, _addr(parity), count, arr, n, window[0], window[1], _addr(old), _addr(new),
                                                            stream or None), "fastecc_update_parity_batch_window")
        return parity

    def _device_list(self, count, n_writes, max_per_stripe, col0, width):
        """the checked (count, n_writes, max_per_stripe, col0, width) of a device-list call; the window as the window methods check it"""
        count = self._batch_count(count)
        for name, v in (("n_writes", n_writes), ("max_per_stripe", max_per_stripe)):
            if isinstance(v, bool) or not isinstance(v, int):
                raise TypeError(name + " must be an int")
        if n_writes < 0 or n_writes >= 1 << 64:
            raise ValueError("n_writes must be in [0, 2^64)")
        if max_per_stripe < 1 or max_per_stripe > 16:
            raise ValueError("max_per_stripe must be in [1, 16]")
        col0, width = self._read_window(col0, width)
        return count, n_writes, max_per_stripe, col0, width

    def update_batch_device(self, data, parity, count, writes, n_writes, new, status, max_per_stripe=1, stream=0, col0=0, width=None):
        """update_batch with the write list in DEVICE memory: `writes` (a device tensor or address, uint64 entries, 8-byte aligned) holds n_writes
        entries b * k + i or WRITE_NONE (the row is skipped), read when the call's kernels run on `stream`, never by the host.  `status` (one
        uint64 of device memory) is set by the call on the stream: 0 when the list was applied, else (error code as uint32) << 32 | one row at
        fault, and then no word of the pool has been written.  max_per_stripe (1 .. 16) is the caller's promise about the writes one stripe gets.
        col0, width (words; width=None: from col0 to the end of the block) as for update_batch; rows of `new` hold `width` words."""
        count, n_writes, max_per_stripe, col0, width = self._device_list(count, n_writes, max_per_stripe, col0, width)
        _check(lib().fastecc_update_batch_device(self._h, _addr(data), _addr(parity), count, _addr(writes), n_writes, max_per_stripe, col0, width,
                                                 _addr(new), _addr(status), stream or None), "fastecc_update_batch_device")
        return data, parity

    def update_parity_batch_device(self, parity, count, writes, n_writes, new, status, old=None, max_per_stripe=1, stream=0, col0=0, width=None):
        """update_batch_device for the parity alone: the blocks changed from row u of `old` (None: from zero) to row u of `new`."""
        count, n_writes, max_per_stripe, col0, width = self._device_list(count, n_writes, max_per_stripe, col0, width)
        _check(lib().fastecc_update_parity_batch_device(self._h, _addr(parity), count, _addr(writes), n_writes, max_per_stripe, col0, width,
                                                        _addr(old), _addr(new), _addr(status), stream or None), "fastecc_update_parity_batch_device")
        return parity

    def update_batch_set_device(self, data, parity, count, pattern_of, writes, n_writes, new, status, max_per_stripe=1, max_absent=None, stream=0,
                                col0=0, width=None):
        """update_batch_set with the write list AND pattern_of in DEVICE memory: `writes`, `status`, max_per_stripe, col0, width and the rows as for
        update_batch_device; `pattern_of` (a device tensor or address, uint32, `count` entries) is read when the call's kernels run on `stream`,
        never by the host, and only for the stripes that a write names.  max_absent is the caller's bound on the written data blocks that are
        absent under their stripe's pattern (None: n_writes, always safe; 0: a promise that none is): it sizes the reconstruction buffer.  A
        non-zero status — as update_batch_device's, and E_INVAL for a bad pattern_of entry of a touched stripe, E_NOMEM for more absent written
        blocks than max_absent — means that no word of the pool has been written."""
        count, n_writes, max_per_stripe, col0, width = self._device_list(count, n_writes, max_per_stripe, col0, width)
        if max_absent is None:
            max_absent = n_writes
        if isinstance(max_absent, bool) or not isinstance(max_absent, int):
            raise TypeError("max_absent must be an int or None")
        if max_absent < 0 or max_absent >= 1 << 64:
            raise ValueError("max_absent must be in [0, 2^64)")
        _check(lib().fastecc_update_batch_set_device(self._h, _addr(data), _addr(parity), count, _addr(pattern_of), _addr(writes), n_writes,
                                                     max_per_stripe, max_absent, col0, width, _addr(new), _addr(status), stream or None),
               "fastecc_update_batch_set_device")
        return data, parity

    def update_parity_batch_set_device(self, parity, count, pattern_of, writes, n_writes, new, status, old=None, max_per_stripe=1, stream=0, col0=0,
                                       width=None):
        """update_batch_set_device for the parity alone: the blocks changed from row u of `old` (None: from zero) to row u of `new`; of a pattern only
        its lost parity blocks matter."""
        count, n_writes, max_per_stripe, col0, width = self._device_list(count, n_writes, max_per_stripe, col0, width)
        _check(lib().fastecc_update_parity_batch_set_device(self._h, _addr(parity), count, _addr(pattern_of), _addr(writes), n_writes, max_per_stripe,
                                                            col0, width, _addr(old), _addr(new), _addr(status), stream or None),
               "fastecc_update_parity_batch_set_device")
        return parity

    def update_batch_set(self, data, parity, count, pattern_of, writes, new, stream=0, col0=0, width=None):
        """update_batch for a pool whose stripes miss blocks: stripe b under pattern pattern_of[b] of the decode_prepare_set set (PATTERN_NONE,
        or a pattern that loses nothing: whole).  Every PRESENT block of a touched stripe becomes what encode gives for the stripe's true data
        — absent data blocks as decode would rebuild them — with the written blocks replaced; absent blocks are neither read nor written, so a
        later repair_batch_set under the same patterns completes the stripes, and read_batch_set of an absent written block returns its new row.
        A window (col0, width, as for update_batch): the same for the words [col0, col0 + width) alone, the old window of an absent written block
        rebuilt from those columns of the survivors."""
        count = self._batch_count(count)
        window = self._write_window(col0, width)
        keep, po = self._pattern_list(pattern_of, count)
        n, arr = self._block_list(writes)
        if window is None:
            _check(lib().fastecc_update_batch_set(self._h, _addr(data), _addr(parity), count, po, arr, n, _addr(new), stream or None),
                   "fastecc_update_batch_set")
        else:
            _check(lib().fastecc_update_batch_set_window(self._h, _addr(data), _addr(parity), count, po, arr, n, window[0], window[1], _addr(new),
                                                         stream or None), "fastecc_update_batch_set_window")
        del keep
        return data, parity

    def update_parity_batch_set(self, parity, count, pattern_of, writes, new, old=None, stream=0, col0=0, width=None):
        """update_parity_batch that leaves the absent parity blocks of every touched stripe alone (only the parity flags of a pattern matter)."""
        count = self._batch_count(count)
        window = self._write_window(col0, width)
        keep, po = self._pattern_list(pattern_of, count)
        n, arr = self._block_list(writes)
        if window is None:
            _check(lib().fastecc_update_parity_batch_set(self._h, _addr(parity), count, po, arr, n, _addr(old), _addr(new), stream or None),
                   "fastecc_update_parity_batch_set")
        else:
            _check(lib().fastecc_update_parity_batch_set_window(self._h, _addr(parity), count, po, arr, n, window[0], window[1], _addr(old), _addr(new),
                                                                stream or None), "fastecc_update_parity_batch_set_window")
        del keep
        return parity

    def pack_blocks(self, raw, packed, stream=0, mem=MEM_DEVICE):
        """GF.md:72-104: k blocks of block_bytes - 4 arbitrary bytes -> k encodable blocks of block_bytes."""
        _check(lib().fastecc_pack_blocks(self._h, _addr(raw), _addr(packed), mem, stream or None), "fastecc_pack_blocks")
        return packed

    def unpack_blocks(self, packed, raw, stream=0, mem=MEM_DEVICE, count_bad=True):
        """Inverse of pack_blocks; returns the number of blocks that are not packer output (None if not counted)."""
        bad = ctypes.c_uint64()
        _check(lib().fastecc_unpack_blocks(self._h, _addr(packed), _addr(raw), mem, stream or None,
                                           ctypes.byref(bad) if count_bad else None), "fastecc_unpack_blocks")
        return int(bad.value) if count_bad else None

    # ---- introspection used by bench.py ----
    def set_plan(self, plan):
        _check(lib().fastecc_set_plan(self._h, plan), "fastecc_set_plan")

    def plan(self):
        return lib().fastecc_plan_string(self._h).decode()

    def profile(self, on=True):
        _check(lib().fastecc_profile_enable(self._h, int(on)), "fastecc_profile_enable")

    def profile_reset(self):
        _check(lib().fastecc_profile_reset(self._h), "fastecc_profile_reset")

    def set_option(self, name, value):
        _check(lib().fastecc_set_option(self._h, name.encode(), int(value)), "fastecc_set_option")

    def profile_read(self, cap=64):
        """{kernel: (total ms, launches, total algorithmic bytes)} since the last reset."""
        names = (ctypes.c_char_p * cap)()
        ms = (ctypes.c_double * cap)()
        cnt = (ctypes.c_uint64 * cap)()
        nbytes = (ctypes.c_uint64 * cap)()
        n = _check(lib().fastecc_profile_read_bytes(self._h, names, ms, cnt, nbytes, cap), "fastecc_profile_read_bytes")
        return {names[i].decode(): (ms[i], int(cnt[i]), int(nbytes[i])) for i in range(n)}


class ShardedEncoder(Encoder):
    """One stripe in column slabs on several GPUs driven by ONE process (fastecc_create_sharded): slab g =
    words [g*S/G, (g+1)*S/G) of every block lives on ``gpu_ids[g]``; ``gpu_ids[0]`` is the root that holds full
    stripes.  ``encode(data, parity)`` takes full stripes (root device or host memory);
    ``encode_sharded(data_slabs, parity_slabs=None, parity=None)`` takes data that is already sharded."""

    def __init__(self, n, k, block_bytes, gpu_ids, field=FIELD_GF_FFF00001):
        self._h = ctypes.c_void_p()
        self.n, self.k, self.block_bytes, self.field = n, k, block_bytes, field
        self.gpu_ids = list(gpu_ids)
        self.device = self.gpu_ids[0] if self.gpu_ids else 0
        ids = (ctypes.c_int * len(self.gpu_ids))(*self.gpu_ids)
        _check(lib().fastecc_create_sharded(ctypes.byref(self._h), n, k, block_bytes, field, ids, len(self.gpu_ids)),
               "fastecc_create_sharded")

    @property
    def slab_block_bytes(self):
        return self.block_bytes // len(self.gpu_ids)

    def encode_sharded(self, data_slabs, parity_slabs=None, parity=None, stream=0):
        g = len(self.gpu_ids)
        d = (ctypes.c_void_p * g)(*[_addr(x) for x in data_slabs])
        p = (ctypes.c_void_p * g)(*[_addr(x) for x in parity_slabs]) if parity_slabs is not None else None
        _check(lib().fastecc_encode_sharded(self._h, d, p, _addr(parity), stream or None), "fastecc_encode_sharded")
        return parity if parity is not None else parity_slabs

    def encode_sharded_blocks(self, data, parity_blocks, data_is_blocks=False, stream=0):
        """Block-distributed result: parity_blocks[g] receives parity blocks [g*M/G, (g+1)*M/G) whole on GPU g (all-to-all over the peers).
        data[g]: column slab g, or with data_is_blocks the data blocks [g*k/G, (g+1)*k/G) whole."""
        g = len(self.gpu_ids)
        d = (ctypes.c_void_p * g)(*[_addr(x) for x in data])
        p = (ctypes.c_void_p * g)(*[_addr(x) for x in parity_blocks])
        _check(lib().fastecc_encode_sharded_blocks(self._h, d, 1 if data_is_blocks else 0, p, stream or None), "fastecc_encode_sharded_blocks")
        return parity_blocks


MIXED_RADIX_Q = (1, 3, 5, 7, 9, 13, 15)
MIXED_RADIX_PFA_Q = MIXED_RADIX_Q + (21, 35, 39, 45, 63, 65, 91, 105, 117)


def mixed_radix_order(k, pfa=False):
    """Transform order fastecc_create_ex(..., CODE_MIXED_RADIX) picks for k data blocks: the smallest q * 2^m >= k,
    q in {1, 3, 5, 7, 9, 13, 15} (pfa: CODE_MIXED_RADIX_PFA, also 21 ... 117), 1 <= m <= 19 (None if there is none)."""
    best = None
    for q in (MIXED_RADIX_PFA_Q if pfa else MIXED_RADIX_Q):
        for m in range(1, 20):
            if (q << m) >= k and (best is None or (q << m) < best):
                best = q << m
    return best


def plan_describe(k, block_bytes, plan=0):
    """Host-only: the pass plan fastecc_create would pick (no device is touched)."""
    buf = ctypes.create_string_buffer(512)
    _check(lib().fastecc_plan_describe(k, block_bytes, plan, buf, 512), "fastecc_plan_describe")
    return buf.value.decode()


def plan_twiddles(k, block_bytes, plan=0, which=0):
    """Host-only: (level-packed twiddle table as a list of k ints, per-level log2 strides)."""
    n = max(k.bit_length() - 1, 0)
    out = (ctypes.c_uint32 * k)()
    sl = (ctypes.c_int32 * max(n, 1))()
    _check(lib().fastecc_plan_twiddles(k, block_bytes, plan, which, out, sl), "fastecc_plan_twiddles")
    return list(out), list(sl)[:n]


def code_coefficient(n, k, data_block, parity_block, flags=0):
    """Host-only: the weight of data block `data_block` in parity block `parity_block` of the (n,k) code (fastecc_create_ex flags)."""
    out = ctypes.c_uint32()
    _check(lib().fastecc_code_coefficient(n, k, flags, data_block, parity_block, ctypes.byref(out)), "fastecc_code_coefficient")
    return int(out.value)


def gf_mul(x, y): return lib().fastecc_gf_mul(x, y)
def gf_pow(x, e): return lib().fastecc_gf_pow(x, e)
def gf_root(order): return lib().fastecc_gf_root(order)
def gf_inv(x): return lib().fastecc_gf_inv(x)


def gf_berlekamp_massey(syndromes, cap=None):
    """Host-only: the shortest LFSR of `syndromes` over GF(p) as [Lambda_0 = 1, ..., Lambda_L]."""
    n = len(syndromes)
    s = (ctypes.c_uint32 * max(n, 1))(*[int(x) % P for x in syndromes])
    cap = n + 1 if cap is None else cap
    lam = (ctypes.c_uint32 * max(cap, 1))()
    L = _check(lib().fastecc_gf_berlekamp_massey(s, n, lam, cap), "fastecc_gf_berlekamp_massey")
    return [int(lam[i]) for i in range(L + 1)]


# GF((2^61-1)^2) scalars, (re, im) tuples
def _pair(z):
    return (ctypes.c_uint64 * 2)(int(z[0]), int(z[1]))


def gf61_mul(x, y):
    out = _pair((0, 0))
    _check(lib().fastecc_gf61_mul(_pair(x), _pair(y), out), "fastecc_gf61_mul")
    return (int(out[0]), int(out[1]))


def gf61_pow(x, e):
    out = _pair((0, 0))
    _check(lib().fastecc_gf61_pow(_pair(x), e, out), "fastecc_gf61_pow")
    return (int(out[0]), int(out[1]))


def gf61_inv(x):
    out = _pair((0, 0))
    _check(lib().fastecc_gf61_inv(_pair(x), out), "fastecc_gf61_inv")
    return (int(out[0]), int(out[1]))


def gf61_root(order):
    out = _pair((0, 0))
    _check(lib().fastecc_gf61_root(order, out), "fastecc_gf61_root")
    return (int(out[0]), int(out[1]))


def gf61_code_coefficient(n, k, data_block, parity_block):
    """Host-only: the weight (re, im) of data block `data_block` in parity block `parity_block` of the (n,k) code over GF((2^61-1)^2)."""
    out = _pair((0, 0))
    _check(lib().fastecc_gf61_code_coefficient(n, k, data_block, parity_block, out), "fastecc_gf61_code_coefficient")
    return (int(out[0]), int(out[1]))
