/*
 * fastecc.h — C ABI of libfastecc_hip.so: the MI355X (gfx950) NTT Reed-Solomon encode path.
 *
 * This is the drop-in boundary for FastECC's encode hot path.  The reference has no ABI: the path is
 * C++ templates #included into RS.cpp.  Each entry point below names the reference code it replaces
 * (file:line in Bulat-Ziganshin/FastECC); INTEGRATION.md shows the host-side binding.
 *
 * Conventions
 *   - Field: GF(p), p = 0xFFF00001 (RS.cpp:86).  Words are native little-endian uint32, every input
 *     word must be < p (README.md:160-162); every output word is the canonical value in [0,p).
 *   - Code: the reference's (n,k) = (2N,N), N = 2^m, 1 <= m <= 19 (RS.cpp:36,82; GF.md:20).  A "block" is
 *     block_bytes/4 consecutive words; a stripe is N blocks back to back (block-major), exactly the
 *     layout RS.cpp:28-33 builds.  parity block j = f(w_2N^(2j+1)) where f interpolates the data
 *     blocks at the powers of w_N = 19^((p-1)/N)   (RS.cpp:40-63).  Other (n,k) — see fastecc_create — evaluate the same
 *     f on other points; a second field (FASTECC_FIELD_GF_P61_SQUARED) exists for 64-bit words.
 *   - All functions return FASTECC_OK (0) or a negative FASTECC_E_* code; no exceptions cross the
 *     ABI and nothing is printed.  The reference returns void and has no error path (RS.cpp:26 prints
 *     and returns on allocation failure); preconditions it leaves implicit are checked here.
 *   - A context is bound to one HIP device (fastecc_create) or to a set of devices (fastecc_create_sharded) and
 *     one (n,k,block_bytes).  Calls on one context are serialised internally (a second thread blocks until the
 *     first call has returned) and nothing about a call is kept in the context, so a context may be shared
 *     between threads and streams; device work of calls that go through the context's internal buffers is
 *     ordered between streams by the library.  Distinct contexts are independent.
 *   - There is NO CPU fallback: without a usable HIP device fastecc_create fails with
 *     FASTECC_E_DEVICE.
 */
#ifndef FASTECC_H
#define FASTECC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FASTECC_VERSION 470 /* 0.4.7: fastecc_update_batch_set_device, fastecc_update_parity_batch_set_device (degraded writes from a write list in device memory) */
/* The version before, for code that tests for it: "#define FASTECC_VERSION 460" was 0.4.6, fastecc_read_batch_set_device and fastecc_read_batch_device
 * (degraded reads from a request list in device memory). */

enum {
    FASTECC_OK = 0,
    FASTECC_E_INVAL = -1,       /* bad argument (n != 2k, k not a power of two, block_bytes % 4, null pointer, ...) */
    FASTECC_E_NOMEM = -2,       /* host or device allocation failed */
    FASTECC_E_DEVICE = -3,      /* no HIP device / HIP runtime error */
    FASTECC_E_UNSUPPORTED = -4, /* field or size outside what GF(0xFFF00001) admits (k > 2^19), or an entry point the
                                   context kind does not offer */
    FASTECC_E_UNCORRECTABLE = -5 /* fastecc_locate_errors / fastecc_correct: the corrupted blocks could not be located */
};

enum {
    FASTECC_FIELD_GF_FFF00001 = 0,   /* the only field RS.cpp instantiates (RS.cpp:86) */
    /*
     * GF(p^2), p = 2^61 - 1: the "64-bit field" of the 64 KB-block configuration.  The reference has NO code for
     * it (README.md:178 and GF.md:30-31 only name the idea; GF(2^61-1) itself has no roots of unity of order
     * > 2), so the conventions are defined HERE and nothing upstream pins them:
     *   - an element is (re, im) = two consecutive little-endian uint64 words, i^2 = -1, both words < p;
     *     a block of block_bytes bytes holds block_bytes / 16 elements (block_bytes % 16 == 0);
     *   - roots of unity: w_(2^62) = (4 + i)^(2^60 - 1)  (4 + i is the first non-square a + i), the root of
     *     order 2^t is w_(2^62)^(2^(62-t)); so w_4 = i and w_8 = 2^30 (1 + i);
     *   - the encoder is the same composition as RS.cpp:40-63 over this field: parity block j is the value at
     *     w_2N^(2j+1) of the polynomial of degree < N whose value at w_N^i is data block i.
     * Supported by create/destroy/encode/encode_blocks/ntt/check_range/decode_prepare/decode/repair/profile/plan_string/gf61_binary and
     * fastecc_set_plan (0 = default: LDS tiles; 1..4 = register passes with that many radix-2 levels; 10+L / 20+L = tiles with a
     * 64 / 128 KiB exchange buffer); the 32-bit-word entry points
     * (scale_blocks, gf_binary, set_option other than "decode_direct_max" and "decode_split") return FASTECC_E_UNSUPPORTED.
     * Codes: (2k,k) with k = 2^m, 1 <= m <= 24, run on the caller's stripes.  Any other k <= 2^24 with n - k <= N = 2^ceil(log2 k) follows
     * the rules fastecc_create documents for GF(0xFFF00001) — the data zero-extended to N blocks, parity block j = block j * 2^fold of the
     * (2N,N) parity, fold = min(log2 N - ceil(log2(n-k)), 4) — through padded copies of the stripes inside the context (two N-block work
     * stripes: encode, decode_prepare, decode and repair on device memory, encode also on host memory; not encode_columns / ntt /
     * check_range).  n = 4k and n = 8k with k = 2^m (more parity than data blocks, fastecc_create's coset rule and nesting order with this
     * field's roots: w_2k; w_4k, w_4k^3; w_8k, w_8k^3, w_8k^5, w_8k^7) are native transforms — the DIF half once into a k-block work stripe
     * of the context, MID and the DIT half once per coset: fastecc_encode on device and host memory (out of place only), set_plan, profile,
     * and decode_prepare / decode / repair on device and host memory: the decoder's scheme on the n-th roots of unity, any n - k lost blocks
     * (one transform of n points; neither the few-loss direct path nor the even / odd split, which are the (2k,k) code's).
     */
    FASTECC_FIELD_GF_P61_SQUARED = 1
};
enum {
    FASTECC_MEM_HOST = 0,        /* ordinary host memory: staged through HBM with copies, the call is synchronous */
    FASTECC_MEM_DEVICE = 1,      /* device memory of the context's device */
    /* pinned host memory (hipHostMalloc / hipHostRegister): fastecc_encode pipelines the stripe through HBM in column
     * slabs — strided copy-engine uploads, kernels and downloads of different slabs overlap, using both directions of the
     * link at once — and is asynchronous on `stream` like FASTECC_MEM_DEVICE.  n = 2k over GF(0xFFF00001) only; the
     * other entry points treat this kind as invalid. */
    FASTECC_MEM_HOST_PINNED = 2
};

typedef struct fastecc_ctx fastecc_ctx;

/* Human-readable text for an error code. */
const char *fastecc_strerror(int code);
/* Which HIP call failed behind the last FASTECC_E_DEVICE / _NOMEM on this thread ("" if none). */
const char *fastecc_last_error_detail(void);
int fastecc_version(void);

/*
 * Create an encoder for (n,k) with `block_bytes`-byte blocks on HIP device `device`.
 * Replaces the set-up part of EncodeReedSolomon<T,P>(N,SIZE) (RS.cpp:22-37) plus the per-call root
 * tables MFA_NTT rebuilds (ntt.cpp:397-402) and the per-block GF_Pow of RS.cpp:51-54: all twiddle
 * tables are built once here and live in HBM.
 * Requires block_bytes > 0 and a multiple of 4, 1 <= k <= 2^19 and n > k.  With N = the smallest power of two >= k:
 *   n = 2k, k = N          the reference's configuration (RS.cpp:22): parity block j = f(w_2k^(2j+1));
 *   n = k + N/2^d, d<=4    fewer parity blocks (RS.md:13-33 "output some M values"): parity block j is block j*2^d of
 *                          the (2N,N) parity, i.e. f on the coset w_2N * <w_(N/2^d)>.  The DIF half is unchanged, the
 *                          evaluation half shrinks to a size-(n-k) transform;
 *   n = 4k or 8k, k = N    more parity blocks (needs n <= 2^20): the n - k parity blocks are f on the 2^e - 1 cosets of
 *                          the data points inside the n-th roots of unity, k blocks per coset, ordered so that codes
 *                          nest: w_2k (= the (2k,k) parity), w_4k, w_4k^3, w_8k, w_8k^3, w_8k^5, w_8k^7; block j of coset
 *                          g is f(g * w_k^j).  parity == data (in place) and fastecc_encode_blocks are not possible;
 *   any other k, n-k <= N  zero extension, exactly RS.md:23-33: the k data blocks are the first k of N (blocks k..N-1 are
 *                          zero and never exist in memory), M = max(N/16, 2^ceil(log2(n-k))) parity blocks of the
 *                          (N + M, N) code above are computed and the first n - k of them are the parity (no extra
 *                          copies: the first and last kernels bound their reads / writes to the existing blocks).
 *                          GF(0xFFF00001) only; encode, encode_blocks, check_range and decode (no ntt / scale_blocks /
 *                          pack / encode_batch).
 * `parity` buffers hold n - k blocks.  Codes with n - k <= 160 (GF(0xFFF00001), option "encode_direct_max") are encoded without the
 * transform — one read of the data, the parity blocks being a dense product of the data with a weight matrix, on the matrix cores (or, for
 * rows they cannot take, up to 32 parity blocks on the VALU); the parity is the same.
 */
int fastecc_create(fastecc_ctx **out, uint64_t n, uint64_t k, uint64_t block_bytes, int field, int device);
/*
 * fastecc_create with flags.  FASTECC_CODE_MIXED_RADIX: the transform order is the smallest N1 = q * 2^m >= k with q in
 * {1, 3, 5, 7, 9, 13, 15} instead of the next power of two — the reference's roadmap for block counts that are not powers of two
 * (NTT.md:43-46, README.md:175; its NTT3 / NTT9 codelets, ntt.cpp:25-146, are never reached by its drivers).  The data
 * points are then the powers of w_N1 = 19^((p-1)/N1) and parity block j = f(w_(2 N1)^(2j+1)): the composition of
 * RS.cpp:40-63 with N1 for N (k < N1: zero extension as in RS.md:23-33; the first n - k <= N1 of the N1 parity blocks
 * are the parity).  With q = 1 this IS fastecc_create; otherwise it is a different code than the zero-extended power-of-
 * two one fastecc_create builds for the same (n,k) — a stripe must be decoded with the flags it was encoded with.
 * k <= 15 * 2^19.  GF(0xFFF00001); encode, encode_blocks, check_range, set_plan, profile, and decode_prepare / decode / repair
 * (orders above 2^20: patterns of up to 2^20 erasures — the locator's product tree needs w_T for its T padded roots and this field
 * stops at order 2^20; patterns of at most 256 lost blocks do not use the tree at any order).  The odd-radix
 * level is fused into the outermost tile passes where a shape exists (2^m with m <= 16..18 depending on q: three trips through
 * HBM, like the power-of-two orders; option "fuse_radix" = 0 gives it its own two passes); measured against zero extension in
 * profiles/r02/mixed_radix_bench.jsonl: faster than zero extension for q <= 9.
 */
#define FASTECC_CODE_MIXED_RADIX 1u
/* The same with the composite odd factors of the prime-factor map as well (NTT.md:43-46 "PFA NTT as well as NTT kernels of orders
 * 3,5,7,9,13"): q in {1, 3, 5, 7, 9, 13, 15, 21, 35, 39, 45, 63, 65, 91, 105, 117}, again the smallest q * 2^m >= k — the next order is
 * then at most 8.4 % above k (20 % with the seven q of FASTECC_CODE_MIXED_RADIX).  The q-point transforms are prime-factor compositions of
 * the 3-, 5-, 7-, 9- and 13-point ones, in registers (3 * 7, 5 * 7, 3 * 13, 9 * 5, 9 * 7, 5 * 13, 7 * 13, 15 * 7, 9 * 13: no twiddles
 * between the two factors).  Three trips through HBM up to m = 10, and for q <= 63 up to m = 13 (q = 63), 14 (35, 39, 45) or 16 (21) (the fused outer tile);
 * beyond that the odd-radix level has its own two passes.  A different code than FASTECC_CODE_MIXED_RADIX builds whenever the orders differ; the
 * other 8 odd divisors of 4095 (195 ... 4095: that many blocks per lane do not fit the registers) are not offered. */
#define FASTECC_CODE_MIXED_RADIX_PFA 4u
/* A/B experiment (same code, same results as fastecc_create): for n = 2k, k = 2^m >= 2^12 the top level of the transform is handled
 * like an odd radix with q = 2 — fused with the next levels in mixed_kernels.hip's kernel instead of tile_kernels.hip's outer tile. */
#define FASTECC_CODE_TOP_RADIX2 2u
int fastecc_create_ex(fastecc_ctx **out, uint64_t n, uint64_t k, uint64_t block_bytes, int field, int device, unsigned flags);
void fastecc_destroy(fastecc_ctx *ctx);

/*
 * encode(n,k,block_bytes, data -> parity).  Replaces the timed lambda RS.cpp:39-67:
 *     MFA_NTT(data,N,SIZE,true); block_i *= root(2N)^i / N; MFA_NTT(data,N,SIZE,false);
 * data   : k blocks, block-major, k*block_bytes bytes (read only unless parity == data)
 * parity : n - k blocks (k for the reference's (2k,k) code), same layout; parity == data gives the reference's in-place behaviour
 *          and needs n - k <= k.  Codes with few parity blocks are evaluated directly (option "encode_direct_max"), same bits.
 * mem_kind FASTECC_MEM_DEVICE: both pointers are device memory on the context's device; the work is
 *          enqueued on `stream` (a hipStream_t, NULL = default stream) and the call does not
 *          synchronise — not even the first call on a context: its twiddle tables are written by a kernel on `stream` in front of the
 *          first pass (a use on another stream later waits for that kernel on the device), so calls may be captured into a hipGraph.  FASTECC_MEM_HOST: pointers are host memory; the call stages through HBM and
 *          returns when `parity` is complete.
 * A stripe is not cut into several launches, and a dispatch holds fewer than 2^32 work-items.  A transform pass takes one wave (64 work-items) per
 * 64-word piece of a block (256-word where rows are 16-byte aligned) and group of 2 to 32 blocks, so only stripes of tens of GiB come near that;
 * one that would need more in a pass is refused with FASTECC_E_UNSUPPORTED — by the power-of-two GF(0xFFF00001) codes before any device work.
 */
int fastecc_encode(fastecc_ctx *ctx, const void *data, void *parity, int mem_kind, void *stream);

/*
 * The same for the word columns [col0_words, col0_words + width_words) of every block only (DEVICE memory, both
 * pointers are the stripes' base addresses).  The columns of a stripe are independent transforms (ntt.cpp:348-350),
 * so a host can cut a stripe into column slabs and overlap their encodes with whatever moves the slabs — which is
 * what fastecc_encode does for FASTECC_MEM_HOST_PINNED stripes and fastecc_encode_sharded for the xGMI gather.
 * n = 2k = 2^m in either field (the 64-bit field: ranges of whole 16-byte elements, i.e. multiples of 4 words);
 * FASTECC_E_UNSUPPORTED for the other codes (they work through whole-stripe scratch buffers), and the caller encodes the
 * stripe in one piece.  Any range is accepted; multiples of 32 words keep every 128-byte row segment whole.
 */
int fastecc_encode_columns(fastecc_ctx *ctx, const void *data, void *parity, uint64_t col0_words, uint64_t width_words, void *stream);

/*
 * One stripe on several GPUs (BASELINE configs[3]; the reference has no multi-device code — SURVEY.md §8e).
 * The word columns of a stripe are independent transforms, so GPU g of G takes words [g*S/G, (g+1)*S/G) of EVERY
 * block (S = block_bytes/4): a "column slab" of k blocks x block_bytes/G bytes, encoded by an ordinary per-device
 * context with no communication; the only exchange is moving slabs (xGMI peer copies, or each GPU's own host link).
 *
 *   fastecc_create_sharded : gpu_ids[0] is the ROOT device.  block_bytes must divide by 4*n_gpus (16*n_gpus for the
 *       64-bit field).  Ids may repeat (several slabs on one device; used by the single-GPU tests).  Every device
 *       must be able to access the root's memory (hipDeviceCanAccessPeer), else FASTECC_E_UNSUPPORTED.  All (n,k)
 *       of fastecc_create are accepted.  One host process drives all devices; for one-process-per-GPU hosts see
 *       fastecc_encode_columns and fastecc_amd/sharding.py (RCCL gather).
 *   fastecc_encode on such a context, same arguments as ever:
 *       FASTECC_MEM_DEVICE       data / parity are full stripes in the ROOT device's memory.  Slab g is pulled by GPU g
 *                                with a strided peer copy, encoded, and its parity pushed back into `parity`; enqueued
 *                                on internal streams, the call behaves as one operation on `stream` (a stream of the
 *                                root device) and does not synchronise.
 *       FASTECC_MEM_HOST_PINNED  full stripes in pinned host memory: every GPU moves its own slab over its own host
 *                                link (strided copies), so G links work in parallel and no xGMI traffic exists.
 *       FASTECC_MEM_HOST         the same for pageable memory, synchronous: every slab has a host thread that moves its columns through that
 *                                slab's rings of pinned slots (128 MiB of pinned memory per GPU), all slabs side by side.
 *   fastecc_encode_sharded : the data is ALREADY sharded — data_slabs[g] is slab g ([k][block_bytes/G], contiguous)
 *       in GPU g's memory.  parity_slabs (optional): G device pointers, slab g of the parity stays on GPU g.
 *       parity (optional): full parity stripe in the ROOT's memory, gathered over xGMI ("a final gather").  At least
 *       one of the two; with parity_slabs == NULL the library uses its own slab buffers.
 *   Both pipeline in column sub-slabs ("sub_slabs" option, default 2; 64 words at 4 KB blocks on 8 GPUs): the copy of
 *   one sub-slab runs behind the kernels of the next.  "gather_mode": 1 = copy engines (hipMemcpy2DAsync, default),
 *   2 = a copy kernel on the sending GPU storing straight into the root's memory.
 *   fastecc_decode_prepare / fastecc_decode / fastecc_repair work on a sharded context as well: a lost block is lost in every
 *   slab, so each slab repairs its own columns with the same pattern; full stripes (root or host memory) are moved slab-wise
 *   like for the encode.
 * Other entry points on a sharded context: destroy, set_option (the two above; anything else is forwarded to every
 * device context), set_plan, plan_string, profile_* (device 0's kernels); the rest return FASTECC_E_UNSUPPORTED.
 */
int fastecc_create_sharded(fastecc_ctx **out, uint64_t n, uint64_t k, uint64_t block_bytes, int field, const int *gpu_ids,
                           int n_gpus);
int fastecc_encode_sharded(fastecc_ctx *ctx, const void *const *data_slabs, void *const *parity_slabs, void *parity, void *stream);
/*
 * The block-distributed form of the same encode — the one that scales.  A gather to one root pushes (G-1)/G of the stripe through ONE
 * GPU's links; here the result stays distributed the way RS.md:13-33 thinks of a codeword (N data and M parity blocks, separately stored
 * units): GPU g ends with parity blocks [g*M/G, (g+1)*M/G) WHOLE in parity_blocks[g] ([M/G][block_bytes], device memory of GPU g).  The
 * exchange is an all-to-all — every GPU sends rows [d*M/G, (d+1)*M/G) of its parity slab into its columns of GPU d's blocks — so each
 * xGMI link carries 1/G^2 of the stripe per direction and no GPU is a hot spot.
 *   data_layout FASTECC_SHARD_SLABS  : data[g] = column slab g on GPU g, as for fastecc_encode_sharded;
 *               FASTECC_SHARD_BLOCKS : the data is block-distributed too — data[g] = data blocks [g*k/G, (g+1)*k/G) whole on GPU g
 *                                      ([k/G][block_bytes]); the mirror all-to-all (whole blocks -> column slabs) runs in front of the
 *                                      encode, sub-slab h+1 travelling while sub-slab h is in the kernels.
 * Needs n - k (and, for FASTECC_SHARD_BLOCKS, k) divisible by the number of GPUs (FASTECC_E_INVAL otherwise) and peer access between every
 * pair of the context's devices (FASTECC_E_UNSUPPORTED otherwise; checked and enabled at the first call).  parity_blocks must not overlap
 * data.  "sub_slabs" and "gather_mode" apply: 2 = one kernel per GPU and sub-slab storing through all peer mappings at once, 1 = G pitched
 * copies on the copy engines, one stream per destination.  Enqueued on internal streams; the call behaves as one operation on `stream`
 * (a stream of the root device) and does not synchronise.
 */
#define FASTECC_SHARD_SLABS 0
#define FASTECC_SHARD_BLOCKS 1
int fastecc_encode_sharded_blocks(fastecc_ctx *ctx, const void *const *data, int data_layout, void *const *parity_blocks, void *stream);
/* Geometry of a sharded context: slabs (= n_gpus given at creation), bytes of a block that one slab holds, and the
 * device of slab g (any pointer may be NULL).  FASTECC_E_INVAL on an ordinary context. */
int fastecc_shard_info(const fastecc_ctx *ctx, int *n_slabs, uint64_t *slab_block_bytes, int *devices, int cap);

/*
 * Many stripes at once: `count` stripes of k blocks stored back to back in DEVICE memory (stripe b at data +
 * b*k*block_bytes, its parity at parity + b*k*block_bytes), encoded by ONE launch per pass.  Same result as `count`
 * fastecc_encode calls; meant for small codes — a (256,128) x 4 KB stripe is 1 MiB and a single launch of it is
 * launch-bound, a batch of them runs at the rate of the large stripes.  n = 2k = 2^m over GF(0xFFF00001) only;
 * parity == data encodes in place; enqueued on `stream` without synchronising.
 * A dispatch holds fewer than 2^32 work-items, so a batch whose passes would take more than 2^24 waves is cut into runs of stripes, each
 * run one launch per pass (a (4,2) x 4 B batch: runs of 2^24 stripes); same bits.  FASTECC_E_UNSUPPORTED, before any device work: count * k
 * beyond 2^31 - 1 blocks, or a code whose single stripe does not fit a dispatch in one of its passes (see fastecc_encode).
 */
int fastecc_encode_batch(fastecc_ctx *ctx, const void *data, void *parity, uint64_t count, void *stream);

/*
 * Writing a pool: `count` stripes in the pool layout of fastecc_decode_batch, in DEVICE memory — stripe b's k data blocks at data +
 * b*k*block_bytes, its n - k parity blocks at parity + b*(n-k)*block_bytes.  Every stripe's parity is, bit for bit, what
 * fastecc_encode(FASTECC_MEM_DEVICE) gives for that stripe alone; `data` is read only and nothing outside the count*(n-k) parity blocks is
 * written.  Every GF(0xFFF00001) code fastecc_encode takes on device memory: (2k,k), n = k + N/2^d, n = 4k / 8k, zero-extended (n,k),
 * mixed radix and PFA.
 *   - Codes of the direct path (n - k <= "encode_direct_max", the rule fastecc_encode applies to one stripe, here to the pool's base
 *     pointers): ONE launch computes the parity of all stripes from the code's weight table when the code has k < 4096 and the launch
 *     fills at least 1024 waves, else the stripes are encoded one by one.  Option "encode_pool_kernel" chooses the kernel (below).
 *   - n = 2k = 2^m beyond the direct path: every transform pass once over the whole pool, as fastecc_encode_batch (and cut into runs of
 *     stripes like it; FASTECC_E_UNSUPPORTED where one stripe alone does not fit a dispatch in a pass).
 *   - Every other code (fold, cosets, zero extension, mixed radix beyond the direct path): fastecc_encode's work stripe by stripe —
 *     correct, not faster than the caller's own loop.
 * Enqueued on `stream` without synchronising, and nothing is staged on the host: steady-state calls are kernels only.  (The first call
 * that takes the direct path builds the code's weight table and waits for it; the matrix-core kernel's fragment table is built on the
 * first such call's stream, and calls on other streams are ordered behind that build on the device.)  The context's call lock is held
 * as for fastecc_encode_batch.
 * FASTECC_E_INVAL, before any device work: a null context, data or parity, count == 0, pointers not 4-byte aligned, byte sizes beyond
 * 64 bits, a parity range that overlaps the data range (no in-place form: stripe b's parity would land on data still to be read).
 * FASTECC_E_UNSUPPORTED: GF((2^61-1)^2), sharded contexts, a set "row_pitch_words".  A refused call writes nothing.
 * fastecc_profile_* scopes: "encode_pool_valu" / "encode_pool_mfma" (one launch each; count*(k + n-k)*block_bytes algorithmic bytes);
 * stripe by stripe: fastecc_encode's own ("direct_encode" or its passes).
 */
int fastecc_encode_pool(fastecc_ctx *ctx, const void *data, void *parity, uint64_t count, void *stream);

/*
 * The reference's own calling form: an array of k HOST block pointers, transformed in place
 * (T** data of RS.cpp:31-33 / ntt.cpp:348-350).  On return blocks[j] holds parity block j (the
 * pointer array itself is left untouched, which is also what two MFA_NTT calls leave behind,
 * SURVEY.md §8 a1).  Synchronous.  The blocks travel through rings of pinned slots that helper threads fill from / empty into
 * the caller's blocks while the copy engine moves the previous slot: k = 2^19 blocks of 4 KB (2 GiB up, 2 GiB down) in 88-110 ms =
 * 39-49 GB/s of data + parity; a table that points into one buffer, block after block (RS.cpp's own), goes up as one copy: 82-88 ms
 * (profiles/r04/encode_blocks_bench.jsonl).
 */
int fastecc_encode_blocks(fastecc_ctx *ctx, void *const *blocks);

/*
 * Length-k number-theoretic transform of the stripe, natural order in and out, unscaled, forward
 * root w_k (inverse != 0: w_k^-1).  Replaces MFA_NTT<T,P>(data,N,SIZE,InvNTT) (ntt.cpp:382-447) and
 * Rec_NTT (ntt.cpp:349-378) followed by reading the blocks through the permuted pointer array.
 * In place on `data` (k*block_bytes bytes).  FASTECC_E_UNSUPPORTED, with `data` untouched, when a pass or the final reordering (one wave per
 * 64-word, or 256-word, piece of every block) would need 2^32 work-items or more in one launch.
 */
int fastecc_ntt(fastecc_ctx *ctx, void *data, int inverse, int mem_kind, void *stream);

/*
 * block i *= scale * base^i for i in [0,k): the per-block twiddle multiply of RS.cpp:51-59
 * (scale = 1/N, base = root(2N)) and, with other arguments, the MFA twiddle of ntt.cpp:421-431.
 * In place on device or host memory as for fastecc_encode.  One launch over the stripe (one wave per 64-word, or 256-word, piece of every
 * block): FASTECC_E_UNSUPPORTED, with `data` untouched, when that would be 2^32 work-items or more.
 */
int fastecc_scale_blocks(fastecc_ctx *ctx, void *data, uint32_t scale, uint32_t base, int mem_kind, void *stream);

/*
 * Element-wise field kernels over `count` words of DEVICE memory (parity tests of the device
 * GF_Mul/GF_Add/GF_Sub against GF(p).cpp:37-48,110-127).  op: 0 = add, 1 = sub, 2 = mul.
 */
int fastecc_gf_binary(fastecc_ctx *ctx, int op, const uint32_t *x, const uint32_t *y, uint32_t *out, uint64_t count,
                      void *stream);

/*
 * The same for the device arithmetic of FASTECC_FIELD_GF_P61_SQUARED (gf61.hpp and the register runs of gf61_kernels.hip), over `count`
 * elements (two uint64 words each: re, im) of DEVICE memory.  That arithmetic keeps words LAZY — congruent to the value and in
 * [0, 2^61 + 2^33), not necessarily canonical — and, inside a run of levels, LOOSE (unfolded 64-bit sums and differences), so the
 * operands here need NOT be canonical and the results are stored as the device function leaves them, with no final reduction: a test
 * checks the residue mod p = 2^61 - 1 AND the output bound.  FASTECC_E_UNSUPPORTED on a GF(0xFFF00001) context; FASTECC_E_INVAL for a null
 * pointer (y may be null where it is unused), an unknown op, or a run op whose count is no multiple of its run length.
 * The op codes exist for tests: more may be added, and they are no part of the encode / decode contract.
 *
 *   op            result (each component)               input domain (each word)                         output bound
 *   ADD           x + y                                 x + y < 2^64 (lazy + lazy: < 2^62 + 2^34)        < 2^61 + 8 (lazy inputs: < 2^61 + 2)
 *   SUB           x - y                                 y <= 2p, x + 2p - y < 2^64 (lazy, lazy)          < 2^61 + 8 (lazy inputs: < 2^61 + 3)
 *   MUL           x * y  in GF(p^2)                     x lazy; y canonical (re, im < p)                 < 2^61 + 8
 *   MUL_RAW       x * y  in GF(p^2)                     x ANY 64-bit word (loose differences reach       < 2^61 + 8
 *                                                       3.5 * 2^62 + 2^34); y canonical
 *   MUL_W8        x * w_8,   w_8 = 2^30 (1 + i)         x lazy                                           < 2^61 + 2^32
 *   MUL_W8I       x * w_8^3                             x lazy                                           < 2^61 + 2^32
 *   MUL_W8_INV    x * w_8^-1                            x lazy                                           < 2^61 + 2^32
 *   MUL_W8I_INV   x * w_8^-3                            x lazy                                           < 2^61 + 2^32
 *   FOLD          x                                     any 64-bit word                                  < 2^61 + 8
 *   CANON         x                                     x <= 2p (every lazy word)                        < p
 *   RUN_DIF + l   2^(l+1)-point forward transform of each run of 2^(l+1) consecutive elements of x, as l + 1 radix-2 decimation-in-
 *   RUN_DIF_INV+l frequency levels (result in bit-reversed order; _INV: with the inverse roots); RUN_DIT + l: the same number of
 *   RUN_DIT + l   decimation-in-time levels with the forward roots (input in bit-reversed order, result in natural order).  l = 0..3.
 *                 These are the register runs every pass is made of (levels that leave loose outputs every other level, w_4 / w_8 /
 *                 w_16 specialised).  x lazy; y unused; count a multiple of 2^(l+1); output < 2^61 + 8.
 */
enum {
    FASTECC_GF61_OP_ADD = 0,
    FASTECC_GF61_OP_SUB = 1,
    FASTECC_GF61_OP_MUL = 2,
    FASTECC_GF61_OP_MUL_RAW = 3,
    FASTECC_GF61_OP_MUL_W8 = 4,
    FASTECC_GF61_OP_MUL_W8I = 5,
    FASTECC_GF61_OP_MUL_W8_INV = 6,
    FASTECC_GF61_OP_MUL_W8I_INV = 7,
    FASTECC_GF61_OP_FOLD = 8,
    FASTECC_GF61_OP_CANON = 9,
    FASTECC_GF61_OP_RUN_DIF = 16,     /* + l, l = 0..3: l + 1 levels */
    FASTECC_GF61_OP_RUN_DIF_INV = 20, /* + l */
    FASTECC_GF61_OP_RUN_DIT = 24      /* + l */
};
int fastecc_gf61_binary(fastecc_ctx *ctx, int op, const uint64_t *x, const uint64_t *y, uint64_t *out, uint64_t count,
                        void *stream);

/*
 * Count the words of a stripe that are not field elements (>= p).  The reference documents "all words < p"
 * as a precondition (README.md:160-162) and never checks it; a host can call this before encoding
 * untrusted data.  Synchronises `stream`.  *bad_words == 0 means the stripe is encodable.
 */
int fastecc_check_range(fastecc_ctx *ctx, const void *data, int mem_kind, void *stream, uint64_t *bad_words);

/*
 * Erasure decoding: recover the erased DATA blocks from any k or more surviving blocks of the codeword.  Both fields:
 * GF(0xFFF00001) as described below; GF((2^61-1)^2) for its (2k,k) codes with the same scheme on 16-byte elements
 * (gf61_decode.hip).  The reference describes the algorithm (README.md:102-119 "Fastest", RS.md:42-79: erasure locator l,
 * p = f*l known everywhere, f(e) = p'(e) / l'(e)) and does not implement it; the data-parallel part here is one
 * transform pipeline of size 2N (the encoder's kernels, N = 2^ceil(log2 k)) between a gather and a scale pass — for
 * the codes with n <= 2k and k >= 2^17 as two pipelines of size k, the data half and the few parity blocks a pattern needs
 * (option "decode_split").
 * Works for every GF(0xFFF00001) code fastecc_create accepts: a code is f on a subset of the (N << e)-th roots of unity
 * (e = 1, or 2 / 3 for n = 4k / 8k); positions that hold none of its blocks count as erased, zero-extended data blocks
 * as known, so exactly n - k losses are tolerated.  Mixed-radix codes (fastecc_create_ex) are decoded the same way on the
 * (2 q 2^m)-th roots of unity with mixed-radix transforms, for orders q 2^m <= 2^20.
 *   fastecc_decode_prepare : set the erasure pattern, k data flags and n - k parity flags (non-zero = block survives).
 *                            The host classifies the positions; the locator's product tree, its two size-NC transforms
 *                            and the inversions run on the device (2.2-2.4 ms at (2^20,2^19); the first call also builds the
 *                            decoder's contexts).  Synchronous.  FASTECC_E_INVAL if fewer than k blocks survive.
 *                            Reusable for any number of stripes.
 *   fastecc_decode         : data (k blocks; the erased ones are overwritten with the recovered content, the others
 *                            are not written) and parity (n - k blocks, read only; content of erased blocks is ignored).
 *                            DEVICE pointers: enqueued on `stream`, no synchronisation.  HOST / HOST_PINNED: staged, synchronous (on sharded contexts
 *                            too) — the data
 *                            stripe and the parity blocks the decoder reads travel up, the rebuilt blocks back (whole stripes
 *                            when more than an eighth of the codeword is lost).
 * fastecc_decode leaves erased parity blocks alone; fastecc_repair rebuilds them too.
 * Patterns with at most 256 lost blocks (option "decode_direct_max", 0..256, default 256; 32 for GF((2^61-1)^2)) take a direct path: every
 * lost block is a fixed linear combination of surviving ones, so prepare builds weight tables (0.2-3.5 ms, no transform contexts) and decode
 * is one read of the data plus a few parity blocks — 0.4 ms for up to 16 lost blocks of a 2 GiB stripe, 0.7 ms for 64, 2.6 ms for 256 (matrix
 * cores; option "direct_kernel") against 3.8-5.7 ms on the transform path (repair: the lost parity blocks in the same pass when at most 32 blocks are lost in all, else in a second read); every GF(0xFFF00001)
 * code, and the (2k,k) codes of GF((2^61-1)^2); identical results.  n = 4k / 8k over GF((2^61-1)^2): the data and the first coset are a (2k,k) code,
 * and up to 32 losses among THOSE 2k blocks (lost blocks of the other cosets do not count; repair re-encodes them) take that code's direct path.
 */
int fastecc_decode_prepare(fastecc_ctx *ctx, const uint8_t *data_present, const uint8_t *parity_present);
int fastecc_decode(fastecc_ctx *ctx, void *data, const void *parity, int mem_kind, void *stream);
/* fastecc_decode, then the erased PARITY blocks as well: the repaired data is encoded once more and the lost parity blocks
 * (only those) are written into `parity` — the whole codeword is whole again ("repair").  Same arguments otherwise. */
int fastecc_repair(fastecc_ctx *ctx, void *data, void *parity, int mem_kind, void *stream);
/*
 * Many stripes, one erasure pattern (rebuilding a failed device: every stripe lost the same blocks).  Same result as `count` calls of
 * fastecc_decode / fastecc_repair with FASTECC_MEM_DEVICE, using the pattern of the last fastecc_decode_prepare for every stripe.
 * Stripes lie back to back in DEVICE memory: stripe b's k data blocks at data + b*k*block_bytes, its n - k parity blocks at
 * parity + b*(n-k)*block_bytes (for (2k,k) codes the layout of fastecc_encode_batch).  Only erased blocks are written;
 * fastecc_decode_batch leaves erased parity blocks alone.  Enqueued on `stream`, no synchronisation.  Every GF(0xFFF00001) code
 * fastecc_decode takes on device memory: (2k,k), n = k + N/2^d, n = 4k / 8k, zero-extended (n,k), mixed radix.
 *   - Patterns of the direct path (at most "decode_direct_max" losses) run each pass over ALL stripes in one launch when the pass reads fewer than
 *     4096 blocks and the batch fills the GPU (count * block_bytes / 4 words make at least 1024 waves of 64 lanes); otherwise direct pass by direct
 *     pass, stripe by stripe.  Option "decode_batch_kernel" (0 = choose, 1 = the batched kernel always, 2 = stripe by stripe), at call time.
 *   - Patterns of the transform path (more losses) are decoded stripe by stripe: correct, but no faster than the caller's own loop.
 * FASTECC_E_INVAL: null or misaligned (not 4-byte) pointers, count == 0, byte sizes beyond 64 bits, no prepared pattern.
 * FASTECC_E_UNSUPPORTED: GF((2^61-1)^2), sharded contexts, a set "row_pitch_words".  A refused call does no device work and writes
 * nothing.  A pattern with nothing to do (no lost data for decode, no lost block for repair) returns FASTECC_OK at once.
 */
int fastecc_decode_batch(fastecc_ctx *ctx, void *data, const void *parity, uint64_t count, void *stream);
int fastecc_repair_batch(fastecc_ctx *ctx, void *data, void *parity, uint64_t count, void *stream);
/*
 * Many stripes, an erasure pattern PER STRIPE (rebuilding a failed device of a pool with rotated placement: stripe b keeps block i on device
 * (i + b) mod n, so one lost device costs stripe b a different block, n patterns in all, and the stripes of one pattern lie n apart).
 *   fastecc_decode_prepare_set : stores a SET of n_patterns erasure patterns in the context.  Pattern q's flags are data_present[q*k .. q*k+k)
 *       and parity_present[q*(n-k) .. q*(n-k)+(n-k)), non-zero = the block survives, as for fastecc_decode_prepare.  The set is independent of
 *       the single prepared pattern: fastecc_decode_prepare, _decode, _repair, _decode_batch, _repair_batch and fastecc_correct* neither read nor
 *       change it, and the set calls neither read nor change the single pattern.  Synchronous: one table build and one synchronisation per
 *       pattern, and a wait for device work that still uses the previous set.  The new set is built aside and swapped in on success: a refused
 *       or failed call leaves the previous set in force.  n_patterns == 0 clears the set and frees its tables.
 *       Limits: n_patterns <= 4096; every pattern loses at most 16 blocks in all (data + parity) and keeps at least k.  Such a pattern is
 *       exactly ONE direct pass of at most 16 outputs: data and parity lost -> both in one pass, only data or only parity lost -> that pass.
 *       A pattern that loses nothing is allowed (its stripes are not touched).  Option "decode_direct_max" does not apply to sets: it tunes the
 *       single pattern's choice between two paths that give the same bits, and a set has the direct path only.
 *       FASTECC_E_INVAL: null context, null flag arrays with n_patterns > 0, n_patterns > 4096, a pattern with fewer than k survivors.
 *       FASTECC_E_UNSUPPORTED: a pattern with more than 16 losses, GF((2^61-1)^2), sharded contexts, a set "row_pitch_words".
 *       FASTECC_E_NOMEM: the tables do not fit.
 *   fastecc_repair_batch_set / fastecc_decode_batch_set : the pool layout of fastecc_repair_batch (stripe b's k data blocks at
 *       data + b*k*block_bytes, its n - k parity blocks at parity + b*(n-k)*block_bytes, DEVICE memory).  pattern_of is a HOST array of `count`
 *       entries and may be reused as soon as the call returns: pattern_of[b] < n_patterns treats stripe b with that pattern;
 *       FASTECC_PATTERN_NONE: stripe b is neither read nor written (it may hold anything, words >= p included).  The result for every stripe,
 *       bit for bit, is what fastecc_decode_prepare(that pattern) + fastecc_repair (resp. fastecc_decode) gives for the stripe alone.  Only erased
 *       blocks are written; fastecc_decode_batch_set leaves erased parity blocks alone and skips stripes whose pattern lost only parity.  Every
 *       GF(0xFFF00001) code fastecc_repair_batch takes.
 *       The stripes that have work are sorted by the size class of their pattern's pass (1, 2, 4, 8 or 16 outputs, rounded up) and every
 *       non-empty class is ONE launch, whatever the number of patterns in it: one lost device of a rotated pool is one launch.  A block owns
 *       whole waves of 64 lanes (blocks shorter than 64 words leave lanes idle; for one pattern and very short blocks fastecc_repair_batch
 *       remains the tool).  A class whose passes read 4096 blocks or more runs stripe by stripe instead (correct, the matrix cores from there
 *       on, no faster than a loop).  Option "decode_batch_kernel" at call time: 0 = that choice, 1 = the kernel always, 2 = stripe by stripe
 *       always; the same bits in every mode.
 *       Enqueued on `stream`; steady-state calls do not synchronise the device.  The per-call list travels through a pinned host buffer and a
 *       device buffer owned by the context, with the rules of fastecc_update_batch: they grow on demand (a growing call waits for the previous
 *       one), an event guards reuse of the pinned buffer, and the calls cannot be captured into a hipGraph.
 *       FASTECC_E_INVAL, before any device work: null context, data, parity or pattern_of, count == 0, pointers not 4-byte aligned, byte sizes
 *       beyond 64 bits, no set prepared, an entry >= n_patterns that is not FASTECC_PATTERN_NONE.  FASTECC_E_UNSUPPORTED: GF((2^61-1)^2),
 *       sharded contexts, a set "row_pitch_words".  A refused call does no device work and writes nothing.  A call in which no stripe has
 *       anything to do returns FASTECC_OK at once.
 */
#define FASTECC_PATTERN_NONE 0xFFFFFFFFu
int fastecc_decode_prepare_set(fastecc_ctx *ctx, const uint8_t *data_present, const uint8_t *parity_present, uint64_t n_patterns);
int fastecc_decode_batch_set(fastecc_ctx *ctx, void *data, const void *parity, uint64_t count, const uint32_t *pattern_of, void *stream);
int fastecc_repair_batch_set(fastecc_ctx *ctx, void *data, void *parity, uint64_t count, const uint32_t *pattern_of, void *stream);

/*
 * Degraded reads: serving reads of a pool while a device is down.  The requested data blocks — often a sector-sized window of them — go to a
 * compact output buffer; the pool itself is left exactly as it is, and healthy and degraded requests may be mixed in one list, in any order.
 *   Layout: the pool layout of fastecc_decode_batch, DEVICE memory: stripe b's k data blocks at data + b*k*block_bytes, its n - k parity blocks
 *       at parity + b*(n-k)*block_bytes, `count` stripes.  data and parity are read only: no byte of the pool is written by either call.
 *   reads: a HOST array of n_reads pool block indices in the numbering of fastecc_update_batch's `writes`: reads[u] = b*k + i is data block i of
 *       stripe b.  Any order, duplicates allowed; the array may be reused as soon as the call returns.
 *   out: DEVICE memory of n_reads rows of width_words 32-bit words, row u for reads[u]: it receives the words [col0_words, col0_words +
 *       width_words) of the requested block.  Nothing outside these n_reads * width_words words is written.
 *   fastecc_read_batch_set : stripe b is taken under pattern pattern_of[b] of the set stored by fastecc_decode_prepare_set.  pattern_of is a HOST
 *       array of `count` entries; only the entries of stripes that some read names are looked at.  FASTECC_PATTERN_NONE, or a pattern that loses
 *       nothing, means every block of that stripe is present.
 *   fastecc_read_batch : every stripe is taken under the single pattern of the last fastecc_decode_prepare, as by fastecc_decode_batch.  Only
 *       patterns of the direct path are served (up to "decode_direct_max" lost blocks); a pattern prepared for the transform path returns
 *       FASTECC_E_UNSUPPORTED.  A pattern with no lost data block is valid: every request is then a copy.  (A pattern that lost nothing at all
 *       is served whatever "decode_direct_max" was when it was prepared: there is no table to build on either path.)
 *   What a request returns:
 *     - a block that is present under its stripe's pattern: a plain copy of the window out of the pool.  No other block of the stripe is read; the
 *       words are copied as stored, words >= p included.
 *     - a lost data block: the window of that block as reconstructed from the survivors — bit for bit the same words of what
 *       fastecc_decode_prepare(that pattern) + fastecc_decode writes into that block for the stripe alone (exact arithmetic, canonical results).
 *       The content of the stripe's lost blocks, data or parity, has no influence on the result: they may hold anything, words >= p included.
 *   Every GF(0xFFF00001) code fastecc_repair_batch_set takes.  ONE launch per call whatever the number of patterns and size classes among the
 *   requests: a request owns whole waves of 64 lanes over its window, and its wave walks the survivors with the one weight per row that the
 *   requested block needs.  Requests of one stripe that ask for several lost blocks each re-read the survivors.  Patterns with many rows — up to
 *   256 lost blocks, codes with k >= 4096 — are served by the same loop, one wave per 64 to 256 columns walking all rows: correct, not tuned;
 *   fastecc_decode remains the tool for single large stripes.
 *   Enqueued on `stream`; steady-state calls do not synchronise the device.  The request list travels through a pinned host buffer and a device
 *   buffer owned by the context, with the rules of fastecc_update_batch / fastecc_repair_batch_set: they grow on demand (a growing call waits for
 *   the previous one), an event guards reuse of the pinned buffer, and the calls cannot be captured into a hipGraph.  fastecc_decode_prepare and
 *   fastecc_decode_prepare_set wait for reads still in flight before they replace tables.  Neither call changes the prepared pattern, the set,
 *   any scrub state or any option.
 *   n_reads == 0 with otherwise valid arguments returns FASTECC_OK and does nothing.
 *   FASTECC_E_INVAL, before any device work and with nothing written: a null context; a null data, parity, reads or out with n_reads > 0, a null
 *   pattern_of (set form); count == 0; data, parity or out not 4-byte aligned; width_words == 0, or col0_words + width_words beyond the words of a
 *   block; a read index >= count*k; byte sizes beyond 64 bits; an `out` range that overlaps the data or the parity range; no set prepared (no
 *   pattern prepared for fastecc_read_batch); an entry of a named stripe that is >= n_patterns and not FASTECC_PATTERN_NONE.
 *   FASTECC_E_UNSUPPORTED: GF((2^61-1)^2), sharded contexts, a set "row_pitch_words", and for fastecc_read_batch a transform-path pattern.
 */
int fastecc_read_batch_set(fastecc_ctx *ctx, const void *data, const void *parity, uint64_t count, const uint32_t *pattern_of,
                           const uint64_t *reads, uint64_t n_reads, uint64_t col0_words, uint64_t width_words, void *out, void *stream);
int fastecc_read_batch(fastecc_ctx *ctx, const void *data, const void *parity, uint64_t count,
                       const uint64_t *reads, uint64_t n_reads, uint64_t col0_words, uint64_t width_words, void *out, void *stream);
/*
 * Degraded reads from a request list in DEVICE memory: fastecc_read_batch_set / fastecc_read_batch with `reads` — and, in the set form,
 * `pattern_of` — produced on the GPU (a storage stack that batches there, a previous kernel) and no host work in the loop.  The host never
 * dereferences `reads`, `pattern_of` or `status`.
 *   reads   : n_reads entries of device memory, 8-byte aligned.  reads[u] = b*k + i, the window [col0_words, col0_words + width_words) and row u
 *             of `out` mean what they mean for the two calls above, and every row that is written holds, bit for bit, the words the host-list call
 *             writes for the same request.  The pool is never written.  n_reads is the list's capacity: a device-side producer pads a shorter list
 *             with FASTECC_READ_NONE, and row u of `out` of such an entry is neither read nor written.  The list is read when the call's kernels
 *             run, in stream order, not when the call is made.
 *   pattern_of : (set form) `count` entries of device memory, 4-byte aligned, read in stream order like the list; only the entries of stripes that
 *             some request names are looked at.  It is a device array because the host cannot know which stripes a device-made list touches, and
 *             copying `count` entries per call would put the host back into the loop.
 *   status  : one uint64 of device memory, 8-byte aligned, set by the call on `stream`: 0 when every request was served.  Otherwise the high 32
 *             bits hold the error code as (uint32_t)code and the low 32 bits one row u that is at fault (any one of them: the first
 *             compare-and-swap from 0 wins).  FASTECC_E_INVAL: an index >= count*k, or (set form) a pattern_of[b] of a requested stripe that is
 *             neither FASTECC_PATTERN_NONE nor below the set's size.
 *             All or nothing: when status is non-zero, no word of out has been written by the call.
 * The return value covers only what the host can decide without the lists, before any device work and with nothing written: everything
 * fastecc_read_batch_set / fastecc_read_batch refuse without looking at `reads`, with the same codes (a null context, count == 0, null or
 * misaligned data, parity or out, an empty window or one outside the block, byte sizes beyond 64 bits, `out` overlapping the pool, no set or no
 * pattern prepared; GF((2^61-1)^2), sharded contexts, a set "row_pitch_words" and for fastecc_read_batch_device a transform-path pattern are
 * FASTECC_E_UNSUPPORTED); FASTECC_E_INVAL for a null status, for reads or status that are not 8-byte aligned or a pattern_of that is not 4-byte
 * aligned, and for reads, pattern_of or status overlapping `out` or status overlapping either list; FASTECC_E_UNSUPPORTED for n_reads above 2^24
 * (the row field of the status word is 32 bits, and a launch holds 2^24 waves).  n_reads == 0 is FASTECC_OK after those checks, with *status set
 * to 0 on the stream.  FASTECC_OK otherwise means "enqueued": the lists' own faults are reported through *status alone.
 * Streams: in steady state — the same or a smaller n_reads than an earlier call on the context, and the same prepared set or pattern — a call
 * makes no host-device copy and no allocation, waits on no event or stream and touches no pinned memory: it resets *status (hipMemsetAsync),
 * launches and returns.  The first call, a growing call and the first call after a fastecc_decode_prepare[_set] may allocate, copy a small table
 * synchronously and wait, as fastecc_read_batch does.  fastecc_decode_prepare and fastecc_decode_prepare_set wait for reads still in flight
 * before they replace tables.  hipGraph capture is not claimed.
 * Method: one kernel with a lane per request translates the list into the entries of the host-list form's read kernel, in
 * a scratch list of the context; the read kernel's waves then look at the status word and at their entry before they do the host-list form's
 * work.  The boundary between the two launches is what makes "all or nothing" hold.
 */
#define FASTECC_READ_NONE UINT64_MAX /* reads[u] of the two calls below: row u of out is left alone */
int fastecc_read_batch_set_device(fastecc_ctx *ctx, const void *data, const void *parity, uint64_t count,
                                  const uint32_t *pattern_of /* device, count entries */, const uint64_t *reads /* device */, uint64_t n_reads,
                                  uint64_t col0_words, uint64_t width_words, void *out, uint64_t *status /* device */, void *stream);
int fastecc_read_batch_device(fastecc_ctx *ctx, const void *data, const void *parity, uint64_t count, const uint64_t *reads /* device */,
                              uint64_t n_reads, uint64_t col0_words, uint64_t width_words, void *out, uint64_t *status /* device */, void *stream);

/*
 * Error detection and location ("scrub"): find blocks that are present but wrong — bit rot, torn or misdirected writes — which
 * the erasure decoder above cannot, because it only acts on losses the caller names.  The reference implements erasure decoding
 * only (README.md:138); its write-up gives the budget used here: E errors plus W erasures need 2E + W check blocks.
 * GF(0xFFF00001), DEVICE memory, every code fastecc_create accepts: (2k,k), n = k + N/2^d, n = 4k / 8k and zero-extended (n,k).
 * Mixed-radix contexts (fastecc_create_ex), GF((2^61-1)^2), sharded contexts, a set "row_pitch_words" and FASTECC_MEM_HOST /
 * HOST_PINNED return FASTECC_E_UNSUPPORTED; null or misaligned (not 4-byte) pointers FASTECC_E_INVAL before any device work.
 * data = k blocks, parity = n - k blocks, each contiguous, as for fastecc_decode.  Enqueued on `stream`; every call waits for it.
 *   fastecc_verify        : *consistent = 1 iff every word is < p and the blocks form a codeword, else 0.
 *   fastecc_locate_errors : the corrupted blocks as codeword indices (data i -> i, parity j -> k + j), increasing; *count = 0 if
 *                           the codeword is consistent.  At most `cap` are written to `blocks` (may be NULL when cap = 0), *count is
 *                           the full number.  Reads only.
 *   fastecc_correct       : locate, rebuild the located blocks in place with the erasure decoder (fastecc_decode_prepare +
 *                           fastecc_repair: this REPLACES the context's prepared erasure pattern), then verify again with a seed
 *                           derived from `seed`.  Same outputs as fastecc_locate_errors.
 * Guarantee: let b be the number of blocks holding a word >= p (certainly corrupt: they count as known erasures) and t the number
 * of other corrupted blocks.  Location succeeds and is exact whenever 2t + b <= n - k and t <= "locate_max" (fastecc_set_option,
 * 0..4096, default 256 = the direct decode path's limit, so that fastecc_correct repairs in one pass; it bounds the host's
 * Berlekamp-Massey work).  Beyond that the calls return FASTECC_E_UNCORRECTABLE or a located set that explains every syndrome of
 * every fingerprint column — never one that does not.  fastecc_correct writes nothing to data or parity unless the located set
 * does; otherwise it returns FASTECC_E_UNCORRECTABLE with both buffers untouched.  (If t + locate_max < n - k + 1 no other
 * codeword is within locate_max blocks of the input, so t = locate_max + 1 errors always give FASTECC_E_UNCORRECTABLE there.)
 * Method: one read of the codeword computes R = 3 fingerprints per block, F_c[j] = sum_w rho_c[w] r_j[w]
 * mod p, with weights rho_c[w] < 2^20 drawn from `seed` (splitmix64), plus a per-block "word >= p" flag.  F is linear, so the
 * fingerprints of a codeword form a codeword of the same code; they are decoded like one: syndromes by one transform of size
 * NC = N << e, Berlekamp-Massey on the host, root search on the device.
 * Seed and detection bound: a corrupted block whose words are all < p differs from the clean one by a non-zero vector mod p;
 * for each column at most one of the 2^20 values of rho_c at a differing word cancels it, so a column misses it with probability
 * <= 2^-20 over the weights, and all three independent columns with probability <= 2^-60 per block.  Words >= p are caught by
 * the flag always.  The same seed gives the same answer.  fastecc_correct checks its result with a second seed: a block missed
 * by all columns of the first (<= 2^-60) is reported as FASTECC_E_UNCORRECTABLE there, after the located blocks were written.
 *
 * Degraded stripes: fastecc_scrub_erasures names the blocks that are known to be ABSENT — a device is down —
 * for the five scrub calls of this context (fastecc_verify, _locate_errors, _correct, _verify_batch, _correct_batch).  data_present = k
 * flags, parity_present = n - k flags, non-zero = present, exactly as for fastecc_decode_prepare; either pointer may be NULL = every
 * block of that part is present, both NULL (or no absent block) clears the pattern.  The pattern is context state, set under the
 * context's lock and independent of the prepared decode pattern: fastecc_decode_prepare, _decode, _repair and fastecc_correct leave
 * it alone, and it changes nothing they do.  Synchronous; may build the context's scrub state; the host arrays may be reused on
 * return.  FASTECC_E_INVAL: null context, more than n - k absent blocks (the previous pattern stays in force).  FASTECC_E_UNSUPPORTED:
 * the contexts fastecc_verify refuses by kind — GF((2^61-1)^2), sharded, mixed radix; a set "row_pitch_words" is refused by the
 * scrub calls themselves, at call time, as before.  With no pattern set every scrub call behaves exactly as described above.  With
 * W the set of absent blocks, w = |W|:
 *   - absent blocks are never read: they may hold anything, words >= p included, and never count among the b blocks above;
 *   - fastecc_verify / _verify_batch: consistent = 1 exactly when every word of every PRESENT block is < p and some codeword agrees
 *     with all present blocks (w fewer syndromes are checked).  With w = n - k every word below p is explained by some codeword:
 *     nothing can be checked and the answer is 1 unless a present block holds a word >= p.  The batch applies the one pattern to
 *     every stripe (a device that is down) and its answer stays the single-stripe one under the same pattern and seed, bit for bit;
 *   - fastecc_locate_errors returns the corrupted PRESENT blocks (absent ones are not listed); the guarantee becomes
 *     2t + b + w <= n - k with t <= "locate_max", and beyond it the wording above holds unchanged;
 *   - fastecc_correct / _correct_batch: a consistent stripe is left untouched, its absent blocks included (status 0).  When blocks
 *     are located, the located AND the absent blocks are rebuilt in one repair (fastecc_decode_prepare with both sets lost, then
 *     fastecc_repair); the codeword is whole afterwards, so the closing verify runs over all blocks with no erasures.  The returned
 *     list still names the located blocks only; status 1.  Nothing is written on FASTECC_E_UNCORRECTABLE.  To get the absent blocks
 *     of consistent stripes back, use fastecc_repair / fastecc_repair_batch with the same flags.
 */
int fastecc_scrub_erasures(fastecc_ctx *ctx, const uint8_t *data_present, const uint8_t *parity_present);
int fastecc_verify(fastecc_ctx *ctx, const void *data, const void *parity, int mem_kind, void *stream, uint64_t seed, int *consistent);
int fastecc_locate_errors(fastecc_ctx *ctx, const void *data, const void *parity, int mem_kind, void *stream, uint64_t seed,
                          uint64_t *blocks, uint64_t cap, uint64_t *count);
int fastecc_correct(fastecc_ctx *ctx, void *data, void *parity, int mem_kind, void *stream, uint64_t seed, uint64_t *blocks,
                    uint64_t cap, uint64_t *count);
/*
 * Scrubbing a pool: many stripes, laid out back to back as for fastecc_decode_batch — stripe b's k data blocks at data + b*k*block_bytes,
 * its n - k parity blocks at parity + b*(n-k)*block_bytes.  Same codes, memory kind (DEVICE) and refusals as fastecc_verify, and
 * FASTECC_E_INVAL before any device work for null pointers (consistent / status / inconsistent included), count == 0, data or parity
 * not 4-byte aligned, byte sizes beyond 64 bits.  A refused call writes nothing.  Synchronous: ordered after prior work on `stream`.
 *   fastecc_verify_batch  : consistent[b] (host, count bytes) = 1 exactly when fastecc_verify with the same seed reports stripe b
 *                           consistent, else 0; *inconsistent = the number of zeros.  Reads only.
 *   fastecc_correct_batch : fastecc_verify_batch, then what fastecc_correct with the same seed does to each inconsistent stripe — this
 *                           REPLACES the context's prepared erasure pattern; which pattern is left behind is unspecified.  status[b]
 *                           (host, count bytes): 0 = consistent and untouched, 1 = corrected, 2 = uncorrectable (fastecc_correct's
 *                           guarantee and refusal, per stripe); *inconsistent = the number of non-zero entries.  Returns
 *                           FASTECC_E_UNCORRECTABLE if any stripe has status 2, with status filled for every stripe either way.
 *                           Option "correct_batch_mode" (at call time) chooses how: 2 = fastecc_correct on each inconsistent stripe through
 *                           its own pointers, one after the other; 1 = the grouped path: one batched location pass over the inconsistent
 *                           stripes (as fastecc_locate_errors_batch), the located stripes grouped by their lost set (located blocks and
 *                           blocks named absent), one fastecc_decode_prepare and one repair over the group's stripes per distinct set
 *                           (fastecc_repair_batch's choice of kernel, option "decode_batch_kernel" included), and one closing verify
 *                           over all repaired stripes with fastecc_correct's second seed; 0 (default) = the grouped path when at least two
 *                           inconsistent stripes qualify for it, else the loop.  Status bytes and the pool's bytes are the same in every
 *                           mode.  Uncorrectable stripes and consistent stripes are never written.
 *   fastecc_locate_errors_batch : fastecc_locate_errors for every stripe of the pool.  status[b] (host, count bytes): 0 = consistent,
 *                           1 = located, 2 = cannot be located (where fastecc_locate_errors returns FASTECC_E_UNCORRECTABLE); counts[b]
 *                           (host, count words) = the full number of located blocks, 0 for status 0 and 2; blocks[b*cap + i], i <
 *                           min(counts[b], cap), = their codeword indices, increasing, as fastecc_locate_errors lists them (absent blocks
 *                           are not listed) — entries beyond that are not written; *inconsistent = the number of non-zero statuses.
 *                           Reads only.  Returns FASTECC_E_UNCORRECTABLE if any status is 2, with every output filled.  FASTECC_E_INVAL as
 *                           for fastecc_verify_batch, and for a null status or inconsistent, or null blocks or counts with cap > 0.
 *                           The answer of every stripe is the one fastecc_locate_errors gives with the same seed and named erasures.
 * Batched location: the inconsistent stripes are read a second time by a list form of the verify pass that
 * gathers all n - k - w syndromes of every fingerprint column; the host runs fastecc_locate_errors' Berlekamp-Massey decisions per stripe;
 * one root search evaluates all locators; the confirmation checks that every syndrome of every column obeys the chosen locator's
 * recurrence, which holds exactly when fastecc_locate_errors' own confirmation does.  Two synchronisations per chunk, none per stripe.
 * Two kinds of stripes go through the single-stripe code with their own pointers instead, with the same answers: a stripe in which a
 * present block holds a word >= p (those blocks are further known erasures of that stripe alone), and every stripe of a code with
 * n - k - w > 512 (the batched pass gathers every syndrome, so their number is bounded: 512 is twice the default "locate_max").
 * Profile scopes of these paths: "fingerprint_batch_list", "scrub_syndromes_gather", "scrub_root_search_batch", "direct_pass_list".
 * Why the answer is the per-stripe one, bit for bit: the fingerprint of a block depends on its words and the seed only, and the syndrome
 * transform acts on each word column of the fingerprint stripe on its own.  The batch puts stripe b's three fingerprint columns at word
 * columns 4b .. 4b+2 of one stripe of NC rows and runs the single-stripe transform once over all of them: every column sees exactly the
 * numbers fastecc_verify computes for that stripe, and exact arithmetic over GF(p) gives the same coefficients.
 * Chunks: a context takes up to 2^21 / NC stripes (at most 2^16, a power of two; NC = the code's transform length N << e) per chunk, so
 * the fingerprint stripe is at most 32 MiB; option "scrub_batch_chunk" (0 = that, else at most this many, at call time) lowers it.  Per
 * chunk: one fingerprint pass that reads the chunk's codewords once (the fixed erasures' locator is applied as it stores), one transform
 * of NC points over 4B words per row, one syndrome check; then one copy of count flags and one synchronisation for the whole call.  The
 * read of the codewords is the cost that scales; the rest is a few launches per chunk.
 */
int fastecc_verify_batch(fastecc_ctx *ctx, const void *data, const void *parity, uint64_t count, void *stream, uint64_t seed,
                         uint8_t *consistent, uint64_t *inconsistent);
int fastecc_correct_batch(fastecc_ctx *ctx, void *data, void *parity, uint64_t count, void *stream, uint64_t seed, uint8_t *status,
                          uint64_t *inconsistent);
int fastecc_locate_errors_batch(fastecc_ctx *ctx, const void *data, const void *parity, uint64_t count, void *stream, uint64_t seed,
                                uint8_t *status, uint64_t *blocks, uint64_t cap, uint32_t *counts, uint64_t *inconsistent);
/*
 * Scrubbing a DEGRADED pool with rotated placement: absent blocks PER STRIPE.  Stripe b of such a pool keeps block i on
 * device (i + b) mod n, so one lost device costs every stripe a different block and no single fastecc_scrub_erasures pattern fits more than 1/n of
 * the stripes.  Same codes, memory kind (DEVICE) and pool layout as fastecc_verify_batch.
 *   fastecc_scrub_erasures_set : stores a SET of n_patterns absent-block patterns in the context's scrub state.  Pattern q's flags are
 *       data_present[q*k .. q*k+k) and parity_present[q*(n-k) .. q*(n-k)+(n-k)), non-zero = present — the array layout of
 *       fastecc_decode_prepare_set, so a caller passes the same two arrays to both.  A pattern names 0 .. n - k blocks absent (there is no 16-loss
 *       limit: that belongs to the direct decode pass); one that names none asks for a full scrub of its stripes.  Limits: n_patterns <= 4096, and
 *       n_patterns * NC <= 2^24 (NC = the code's transform length N << e: the per-pattern locator tables stay at most 64 MiB), beyond that
 *       FASTECC_E_UNSUPPORTED.  FASTECC_E_INVAL: null context, null flag arrays with n_patterns > 0, n_patterns > 4096, a pattern with more than
 *       n - k absent blocks.  FASTECC_E_UNSUPPORTED also for the contexts fastecc_scrub_erasures refuses: GF((2^61-1)^2), sharded, mixed radix.
 *       n_patterns == 0 clears the set and frees its tables.  Synchronous: one table build and one synchronisation for the whole set; the new set
 *       is built aside and swapped in under the context's lock, and a refused or failed call leaves the previous set in force.  The set is
 *       independent of the single fastecc_scrub_erasures pattern in both directions — the five scrub calls above and fastecc_scrub_fingerprints
 *       neither read nor change the set, the set calls neither read nor change the single pattern — and of both decode pattern states.
 *   fastecc_verify_batch_set : pattern_of is a HOST array of `count` entries and may be reused on return.  pattern_of[b] < n_patterns:
 *       consistent[b] is, bit for bit, what fastecc_scrub_erasures(that pattern) followed by fastecc_verify with the same seed answers for stripe
 *       b alone; absent blocks are never read.  FASTECC_PATTERN_NONE: stripe b is not read at all (it may hold anything, words >= p included),
 *       consistent[b] = 1 and it is not counted.  *inconsistent = the number of zeros in consistent.  Synchronous; reads only.
 *       FASTECC_E_INVAL, before any device work and with nothing written: the refusals of fastecc_verify_batch, a null pattern_of, no set
 *       prepared, an entry >= n_patterns that is not FASTECC_PATTERN_NONE.  FASTECC_E_UNSUPPORTED as for fastecc_verify_batch.  Option
 *       "scrub_batch_chunk" applies.
 *   fastecc_correct_batch_set : fastecc_verify_batch_set, then for each inconsistent stripe what fastecc_scrub_erasures(its pattern) +
 *       fastecc_correct(same seed) does to that stripe alone: locate under that pattern's erasures (2t + b + w <= n - k, t <= "locate_max"),
 *       rebuild located and absent blocks in one fastecc_decode_prepare + fastecc_repair, closing verify over all blocks with the derived seed.
 *       status[b]: 0 = consistent or skipped, untouched, absent blocks included; 1 = corrected, the whole codeword is back; 2 = uncorrectable,
 *       untouched.  *inconsistent = the number of stripes the verify pass flagged.  Returns FASTECC_E_UNCORRECTABLE if any status is 2, with
 *       status filled either way.  REPLACES the context's single prepared decode pattern; which pattern is left behind is unspecified.  The decode
 *       pattern SET, the single scrub pattern and the scrub set are left alone.  Option "correct_batch_mode" (at call time) chooses how, with the
 *       meaning it has for fastecc_correct_batch: 2 = the inconsistent stripes one after the other, each as above; 1 = the grouped path (DESIGN.md
 *       section 27): one batched location pass over the inconsistent stripes (as fastecc_locate_errors_batch_set), the located stripes grouped by
 *       their lost set (located blocks and the blocks absent under the stripe's own pattern), ONE pattern set private to the call built from the
 *       distinct lost sets and one repair launch per size class over all their stripes (fastecc_repair_batch_set's kernel and its choice, option
 *       "decode_batch_kernel" included; lost sets of more than 16 blocks and distinct sets beyond the 4096th of a call go one
 *       fastecc_decode_prepare and one list-form repair per set), and one closing verify over all repaired stripes with fastecc_correct's second
 *       seed; 0 (default) = the grouped path when at least two inconsistent stripes qualify for it, else the loop.  Status bytes, *inconsistent,
 *       the return code and every byte of the pool are the same in every mode.  Uncorrectable and consistent stripes are never written.
 *       Workflow: this call makes the bad stripes whole, then fastecc_repair_batch_set with the same flag arrays and pattern_of brings back the
 *       absent blocks of all the others.
 *   fastecc_locate_errors_batch_set : fastecc_locate_errors_batch with a pattern per stripe; the outputs are those of that call (status 0 / 1 / 2,
 *       counts, blocks[b*cap + i], *inconsistent), written only at the end; FASTECC_E_UNCORRECTABLE if any status is 2, with every output filled.
 *       pattern_of[b] < n_patterns: the answer of stripe b is, bit for bit, what fastecc_scrub_erasures(that pattern) followed by
 *       fastecc_locate_errors with the same seed gives for that stripe alone; absent blocks are never read and never listed.
 *       FASTECC_PATTERN_NONE: the stripe is not read, has status 0 and is not counted.  Reads only.  Refusals, before any device work and with
 *       nothing written: those of fastecc_verify_batch_set (no set prepared, an entry >= n_patterns that is not FASTECC_PATTERN_NONE, a null
 *       pattern_of), and fastecc_locate_errors_batch's on null outputs and on cap.  FASTECC_E_UNSUPPORTED for the contexts
 *       fastecc_scrub_erasures_set refuses.
 * Batched location under the set: the list pass of fastecc_locate_errors_batch with the erasure view per list entry.  Each
 * entry follows fastecc_locate_errors' decisions under its own pattern (n - k - w syndromes, w that pattern's absent blocks); a root at a block
 * absent under the stripe's pattern refuses the stripe.  Through the single-stripe code under the stripe's pattern instead, with the same answers: a
 * stripe in which a present block holds a word >= p, one whose pattern leaves more than 512 syndromes, one whose pattern leaves none.  Stripes of
 * all kinds may share a call and a chunk.
 * Profile scopes: "fingerprint_set" (its bytes: the blocks actually read), "scrub_transform_batch", "scrub_syndromes_set"; of the batched location
 * and the grouped repair: "fingerprint_set_list" (bytes as above), "scrub_syndromes_gather_set", and the reused "scrub_root_search_batch" and
 * "direct_pass_set" (the wide lost sets: "direct_pass_list" / "direct_pass").
 */
int fastecc_scrub_erasures_set(fastecc_ctx *ctx, const uint8_t *data_present, const uint8_t *parity_present, uint64_t n_patterns);
int fastecc_verify_batch_set(fastecc_ctx *ctx, const void *data, const void *parity, uint64_t count, const uint32_t *pattern_of,
                             void *stream, uint64_t seed, uint8_t *consistent, uint64_t *inconsistent);
int fastecc_correct_batch_set(fastecc_ctx *ctx, void *data, void *parity, uint64_t count, const uint32_t *pattern_of,
                              void *stream, uint64_t seed, uint8_t *status, uint64_t *inconsistent);
int fastecc_locate_errors_batch_set(fastecc_ctx *ctx, const void *data, const void *parity, uint64_t count, const uint32_t *pattern_of,
                                    void *stream, uint64_t seed, uint8_t *status, uint64_t *blocks, uint64_t cap, uint32_t *counts,
                                    uint64_t *inconsistent);
/*
 * The fingerprints themselves (tests only, like fastecc_gf_binary: this call is no part of the scrub contract and may change).  It runs the
 * fingerprint pass of the scrub calls above — the same kernels through the same host paths and launch configurations — stops before the
 * syndrome transform and returns what the pass computed, so that a test can compare it with an exact model:
 *   weights : weight word w (w = 0 .. words per block - 1, the same for every block) comes from the w-th output x of splitmix64 started at
 *             state `seed` (state += 0x9E3779B97F4A7C15; z = state; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) *
 *             0x94D049BB133111EB; x = z ^ z >> 31): rho_0 = x & 0xFFFFF, rho_1 = (x >> 20) & 0xFFFFF, rho_2 = (x >> 40) & 0xFFFFF;
 *   F_c     : sum over w of rho_c[w] * r[w] mod p, r[w] the block's 32-bit word as stored (words >= p are not reduced first), canonical.
 * form 0 = the single-stripe pass of fastecc_verify / _locate_errors / _correct (count must be 1, list NULL); 1 = the batch pass of
 * fastecc_verify_batch over the stripes 0 .. count-1 of a pool, in its chunks (option "scrub_batch_chunk" applies; list NULL); 2 = the list
 * pass of fastecc_locate_errors_batch / _correct_batch over the stripes list[0 .. count) of the pool (list: a host array; a stripe may be
 * named more than once).  out (host, count*n*3 words): out[(i*n + j)*3 + c] = F_c of block j of entry i, block j = data block j for j < k,
 * else parity block j - k.  big (host, count bytes): big[i] = 1 iff some block of entry i holds a word >= p, else 0.  Synchronous.
 * Refusals: those of fastecc_verify / fastecc_verify_batch; FASTECC_E_INVAL also for an unknown form, null out or big, form 0 with
 * count != 1, a list without form 2 or form 2 without one; FASTECC_E_UNSUPPORTED while a fastecc_scrub_erasures pattern is set, and for
 * forms 1 and 2 on a code with fixed erasures (zero-extended and n = k + N/2^d codes: those passes store F times the erasures' locator).
 */
int fastecc_scrub_fingerprints(fastecc_ctx *ctx, const void *data, const void *parity, uint64_t count, const uint64_t *list, int form,
                               void *stream, uint64_t seed, uint32_t *out, uint8_t *big);

/*
 * Small writes: bring the parity up to date after `count` data blocks changed, without reading the rest of the stripe.  The code is
 * linear, so the new parity is the old one plus the weighted changes; the weight of data block i in parity block q is the generator-
 * matrix entry fastecc_code_coefficient gives.  One read-modify-write pass over the parity per 16 changed blocks; the rest of the
 * data is never touched.
 *   fastecc_update        : data is the whole k-block stripe.  Reads the old content of data[blocks[u]], adds its change to parity
 *                           and writes new_blocks[u] (count blocks, contiguous) into the stripe.  Afterwards data and parity are
 *                           exactly what fastecc_encode of the new stripe gives.
 *   fastecc_update_parity : the data blocks live elsewhere: old_blocks and new_blocks are count contiguous blocks each; old_blocks ==
 *                           NULL means zero blocks (incremental encoding: zero the parity, then add blocks as they arrive).
 * Every GF(0xFFF00001) code of fastecc_create / fastecc_create_ex, FASTECC_MEM_DEVICE only.  blocks: a host array of distinct indices
 * < k in any order (it may be reused as soon as the call returns); count = 0 is a no-op and there is no upper limit.  Enqueued on
 * `stream` without synchronising, the first call included (its weight table is built by a kernel on `stream`).  Inputs must be < p;
 * new_blocks / old_blocks must not overlap data or parity.  FASTECC_E_INVAL (before any device work): null pointers with count > 0,
 * an index >= k, a duplicate index, pointers that are not 4-byte aligned.  FASTECC_E_UNSUPPORTED: GF((2^61-1)^2), sharded contexts,
 * a set "row_pitch_words", host memory.  At (2^20, 2^19) x 4 KB an update is cheaper than a fresh fastecc_encode up to 40 changed blocks and dearer at 64.
 */
int fastecc_update(fastecc_ctx *ctx, void *data, void *parity, const uint64_t *blocks, uint64_t count, const void *new_blocks,
                   int mem_kind, void *stream);
int fastecc_update_parity(fastecc_ctx *ctx, void *parity, const uint64_t *blocks, uint64_t count, const void *old_blocks,
                          const void *new_blocks, int mem_kind, void *stream);
/*
 * Small writes into a pool: many stripes stored back to back in DEVICE memory, the layout of fastecc_decode_batch — stripe b's k data
 * blocks at data + b*k*block_bytes, its n - k parity blocks at parity + b*(n-k)*block_bytes, `count` stripes.  There is no mem_kind.
 *   writes     : a host array of n_writes DISTINCT pool block indices in any order; writes[u] = b*k + i is data block i of stripe b.  It
 *                may be reused as soon as the call returns.
 *   new_blocks : n_writes contiguous blocks in device memory, row u for writes[u].  old_blocks (the parity form): the same shape, the
 *                blocks' previous content; NULL means zero blocks (incremental encoding, as for fastecc_update_parity).
 *   fastecc_update_batch        : every touched stripe's data and parity become, bit for bit, what fastecc_encode gives for the new
 *                                 stripe — the result of fastecc_update on each touched stripe with its own writes.
 *   fastecc_update_parity_batch : the same for the parity alone; the data blocks live elsewhere.
 * A stripe that no write names is neither read nor written: it may hold anything, words >= p included.  Inputs of touched stripes must
 * be < p; new_blocks / old_blocks must not overlap data or parity.  Every GF(0xFFF00001) code fastecc_update takes: (2k,k),
 * n = k + N/2^d, n = 4k / 8k, zero-extended (n,k), mixed radix and PFA.  n_writes == 0 with otherwise valid arguments is a no-op.
 * FASTECC_E_INVAL, before any device work: a null context, count == 0, a null parity, writes or new_blocks (or data, for
 * fastecc_update_batch) with n_writes > 0, pointers that are not 4-byte aligned, an index >= count*k, a duplicate index, byte sizes
 * beyond 64 bits.  FASTECC_E_UNSUPPORTED: GF((2^61-1)^2), sharded contexts, a set "row_pitch_words" (and more than (2^32 - 1) / 7 writes in
 * one call).  A refused call writes nothing.
 * Method: the weight table of fastecc_update serves every stripe, so nothing per stripe is built.  The host sorts
 * the writes by (stripe, block) and cuts each stripe's writes into segments of at most 16; segment r of every stripe runs in round r, one
 * launch per padded segment length (1, 2, 4, 8, 16) — the usual pool write, one block per stripe, is ONE launch for the parity plus one
 * that stores the new blocks (fastecc_update_batch only).
 * Streams: enqueued on `stream`; steady-state calls do not synchronise the device.  The sorted list travels through a pinned host
 * buffer and a device buffer owned by the context, both grown on demand: the first call, and a call with a longer list than any before,
 * allocate and may therefore synchronise.  A call made while the previous call's list is still on its way to the device waits on the host
 * for that copy (an event), not for the device; the copy is itself enqueued on its call's stream, behind the work enqueued there before
 * it, so the host runs at most one call ahead of the device.  Because of this host staging the calls cannot be captured into a hipGraph.
 */
int fastecc_update_batch(fastecc_ctx *ctx, void *data, void *parity, uint64_t count, const uint64_t *writes, uint64_t n_writes,
                         const void *new_blocks, void *stream);
int fastecc_update_parity_batch(fastecc_ctx *ctx, void *parity, uint64_t count, const uint64_t *writes, uint64_t n_writes,
                                const void *old_blocks, const void *new_blocks, void *stream);
/*
 * Degraded writes: fastecc_update_batch / fastecc_update_parity_batch for a pool in which stripes miss blocks.  Layout, `writes`, new_blocks and
 * old_blocks are exactly those of the two calls above; pattern_of is exactly that of fastecc_read_batch_set: a HOST array of `count` entries, stripe
 * b is taken under pattern pattern_of[b] of the set stored by fastecc_decode_prepare_set, only the entries of stripes that some write names are
 * looked at, and FASTECC_PATTERN_NONE, or a pattern that loses nothing, means the stripe is whole.  A block is ABSENT when its stripe's pattern says
 * it is lost.
 *   fastecc_update_batch_set : for a touched stripe let X be its true old data — present data blocks as stored, absent ones as
 *       fastecc_decode_prepare(that pattern) + fastecc_decode would rebuild them — and X' be X with the written blocks replaced.  After the call
 *       every PRESENT data block of the stripe holds its block of X', and every PRESENT parity block holds, bit for bit, the parity block
 *       fastecc_encode gives for X'.  No absent block, data or parity, is written, and its content has no influence on anything: it may hold
 *       words >= p.  So a later fastecc_repair_batch_set of the pool under the same patterns leaves every touched stripe bit-identical to a fresh
 *       fastecc_encode of X', and fastecc_read_batch_set of an absent written block returns its new content.  For a whole stripe the result is
 *       bit-identical to fastecc_update_batch.
 *   fastecc_update_parity_batch_set : the data lives elsewhere and the old rows come from old_blocks (NULL: zero), so only the parity flags of a
 *       pattern matter: present parity blocks are updated as by fastecc_update_parity_batch, absent ones are not touched.
 * A stripe that no write names is neither read nor written.  Inputs of touched stripes' PRESENT blocks must be < p.  n_writes == 0 with otherwise
 * valid arguments (a set prepared included) is a no-op.  Neither call changes the pattern set, the single prepared pattern, any scrub state or any
 * option; fastecc_decode_prepare_set waits for a degraded write still in flight before it swaps tables, as it does for reads.
 * Refusals, before any device work and with nothing written.  FASTECC_E_INVAL: everything fastecc_update_batch refuses (a null context, count == 0,
 * null pointers with n_writes > 0, misalignment, an index >= count*k, a duplicate, byte sizes beyond 64 bits), a null pattern_of, no set prepared,
 * an entry of a TOUCHED stripe that is >= n_patterns and not FASTECC_PATTERN_NONE, new_blocks / old_blocks overlapping the pool.
 * FASTECC_E_UNSUPPORTED: GF((2^61-1)^2), sharded contexts, a set "row_pitch_words" (and more than (2^32 - 1) / 10 writes in one call).
 * FASTECC_E_NOMEM: the reconstruction buffer — one block per absent written block, owned by the context and grown on demand — does not fit.
 * Method, two phases on `stream`: the old rows of the absent written blocks are rebuilt into the reconstruction buffer by the
 * kernel of fastecc_read_batch_set (one request each); then update_set_kernel does what the kernel of fastecc_update_batch does, with each old row
 * taken from the pool or from that buffer and the stripe's absent parity blocks skipped (neither loaded nor stored); at the end only present data
 * blocks are stored.
 * Streams: the stream and staging rules of fastecc_update_batch hold word for word — enqueued on `stream`, steady-state calls do not synchronise the
 * device, the staged lists travel through pinned and device buffers owned by the context that grow on demand, an event guards the reuse of the
 * pinned side, and the calls cannot be captured into a hipGraph.
 */
int fastecc_update_batch_set(fastecc_ctx *ctx, void *data, void *parity, uint64_t count, const uint32_t *pattern_of, const uint64_t *writes,
                             uint64_t n_writes, const void *new_blocks, void *stream);
int fastecc_update_parity_batch_set(fastecc_ctx *ctx, void *parity, uint64_t count, const uint32_t *pattern_of, const uint64_t *writes,
                                    uint64_t n_writes, const void *old_blocks, const void *new_blocks, void *stream);
/*
 * Sub-block writes: the four pool calls above for one window of word columns [col0_words, col0_words + width_words) of every written block — a
 * 512-byte sector of a 4 KB block is (col0_words, 128).  One window holds per call; callers group their writes by window.  Each call takes the
 * arguments of its whole-block form with the window in front of the rows.
 *   new_blocks, old_blocks : n_writes ROWS of width_words words, compact at pitch width_words (not blocks): row u belongs to writes[u] and holds
 *       words [col0_words, col0_words + width_words) of that block.  old_blocks == NULL still means zero.
 *   writes, pattern_of, the pool layout, streams and staging keep the meaning they have in the whole-block forms, word for word (the calls still
 *       cannot be captured into a hipGraph).
 * Result for a touched stripe: let X' be the stripe's true data (absent blocks as fastecc_decode would rebuild them) with words
 * [col0_words, col0_words + width_words) of each written block replaced by its row.  Afterwards those columns of every written data block that is
 * PRESENT hold the row (the parity forms store no data), and the same columns of every PRESENT parity block hold, bit for bit, what fastecc_encode gives
 * for X' in those columns.
 * Footprint: no word outside the window's columns is read or written, in any block of the pool; such words may be >= p.  Inside the window the
 * inputs of touched stripes' present blocks must be < p.  Absent blocks and untouched stripes are neither read nor written.  The old window of an
 * absent written block is rebuilt from the window columns of the survivors only (into a buffer of width_words words per such block).
 * With col0_words = 0 and width_words = block_bytes / 4 every call is bit-identical to its whole-block form; on a pool whose words are all < p a
 * window call is bit-identical to the whole-block call given "the old block with the window replaced".  The vector width of the kernels follows
 * the window: 4 words per lane need col0_words, width_words and block_bytes / 4 divisible by 4 and 16-byte aligned pointers (2: by 2, 8 bytes).
 * Refusals, before any device work and with nothing written: everything the corresponding whole-block call refuses, with the same code;
 * FASTECC_E_INVAL for width_words == 0 or col0_words + width_words beyond the block's words (checked without overflow), and for new_blocks or
 * old_blocks (as n_writes * width_words words) overlapping the pool — in all four forms.  n_writes == 0 with otherwise valid arguments is a no-op.
 * Method: one kernel family, update_window_kernel, for the four calls; the parity read-modify-write touches width_words
 * words of every present parity block of a touched stripe instead of the whole block.
 */
int fastecc_update_batch_window(fastecc_ctx *ctx, void *data, void *parity, uint64_t count, const uint64_t *writes, uint64_t n_writes,
                                uint64_t col0_words, uint64_t width_words, const void *new_blocks, void *stream);
int fastecc_update_parity_batch_window(fastecc_ctx *ctx, void *parity, uint64_t count, const uint64_t *writes, uint64_t n_writes,
                                       uint64_t col0_words, uint64_t width_words, const void *old_blocks, const void *new_blocks, void *stream);
int fastecc_update_batch_set_window(fastecc_ctx *ctx, void *data, void *parity, uint64_t count, const uint32_t *pattern_of, const uint64_t *writes,
                                    uint64_t n_writes, uint64_t col0_words, uint64_t width_words, const void *new_blocks, void *stream);
int fastecc_update_parity_batch_set_window(fastecc_ctx *ctx, void *parity, uint64_t count, const uint32_t *pattern_of, const uint64_t *writes,
                                           uint64_t n_writes, uint64_t col0_words, uint64_t width_words, const void *old_blocks,
                                           const void *new_blocks, void *stream);
/*
 * Pool writes from a write list in DEVICE memory: fastecc_update_batch_window / fastecc_update_parity_batch_window with `writes` produced on the
 * GPU (a storage stack that batches there, a previous kernel) and no host work in the loop.  The host never dereferences `writes` or `status`.
 *   writes  : n_writes entries of device memory, 8-byte aligned.  writes[u] = b*k + i and row u of new_blocks / old_blocks (pitch width_words) mean
 *             what they mean for the window calls above; col0_words = 0 and width_words = block_bytes / 4 is the whole block and leaves the bytes of
 *             fastecc_update_batch / fastecc_update_parity_batch.  Every entry that is not FASTECC_WRITE_NONE is a write; n_writes is the list's
 *             capacity, and a device-side producer pads a shorter list with FASTECC_WRITE_NONE (row u of such an entry is not read).  The list is
 *             read when the call's kernels run, in stream order, not when the call is made.
 *   max_per_stripe : the caller's promise about how many writes one stripe gets in this call, 1 to 16 (16 is the pass size of fastecc_update).
 *             It selects the launches: one per padded segment length 1, 2, 4, 8, 16 up to the promise rounded up to a power of two — with the usual
 *             promise of 1 the parity work is ONE launch.  The device form has no rounds: a burst with more than 16 writes to one stripe goes
 *             through the host-list calls (fastecc_update_batch and friends) or a re-encode (fastecc_encode_pool).
 *   status  : one uint64 of device memory, 8-byte aligned, set by the call on `stream`: 0 when the list was applied.  Otherwise the high 32 bits
 *             hold the error code as (uint32_t)code and the low 32 bits one row u that is at fault (any one of them: the first compare-and-swap
 *             from 0 wins).  FASTECC_E_INVAL: an index >= count*k, or two writes to the same block.  FASTECC_E_UNSUPPORTED: a stripe with more than
 *             max_per_stripe writes.  All or nothing: when status is non-zero, no word of the pool has been written by the call.
 * The return value covers only what the host can decide without the list, before any device work and with nothing written: everything
 * fastecc_update_batch_window / fastecc_update_parity_batch_window refuse without looking at the list, with the same codes (a null context, count ==
 * 0, null or misaligned pointers, byte sizes beyond 64 bits, a window outside the block, rows overlapping the pool; GF((2^61-1)^2), sharded contexts
 * and a set "row_pitch_words" are FASTECC_E_UNSUPPORTED); FASTECC_E_INVAL for a null status, max_per_stripe outside 1 .. 16, and writes or status
 * that are not 8-byte aligned or overlap the pool or the rows; FASTECC_E_UNSUPPORTED for count or n_writes above 2^24 (the per-stripe counters are
 * reset by every call: 4 bytes per stripe).  n_writes == 0 is FASTECC_OK after those checks, with *status set to 0 on the stream.  FASTECC_OK
 * otherwise means "enqueued": the list's own faults are reported through *status alone.
 * Streams: in steady state — the same or a smaller n_writes, count and max_per_stripe than an earlier call on the context — a call makes no
 * host-device copy and no allocation, waits on no event or stream and touches no pinned memory: it resets its counters and *status
 * (hipMemsetAsync), launches and returns.  The first call and a growing call allocate the context's scratch and may wait, as
 * fastecc_update_batch does.  hipGraph capture is not claimed.  The _set (degraded) forms of these two calls are
 * fastecc_update_batch_set_device / fastecc_update_parity_batch_set_device, below.
 * Method: the segment tables of update_window_kernel are built by three kernels without a sort — a slot per write from a
 * per-stripe counter, the records, the segments by length class — and the order of a stripe's writes inside its segment, which depends on atomic
 * arrival, has no influence on the result: the sums are exact 96-bit integers reduced once, so any permutation of the list leaves the same bytes.
 */
#define FASTECC_WRITE_NONE UINT64_MAX /* writes[u] of the two calls below: row u is skipped */
int fastecc_update_batch_device(fastecc_ctx *ctx, void *data, void *parity, uint64_t count, const uint64_t *writes /* device */, uint64_t n_writes,
                                uint32_t max_per_stripe, uint64_t col0_words, uint64_t width_words, const void *new_blocks,
                                uint64_t *status /* device */, void *stream);
int fastecc_update_parity_batch_device(fastecc_ctx *ctx, void *parity, uint64_t count, const uint64_t *writes /* device */, uint64_t n_writes,
                                       uint32_t max_per_stripe, uint64_t col0_words, uint64_t width_words, const void *old_blocks /* may be NULL: zero */,
                                       const void *new_blocks, uint64_t *status /* device */, void *stream);
/*
 * Degraded pool writes from a write list in DEVICE memory: fastecc_update_batch_set_window / fastecc_update_parity_batch_set_window with `writes`
 * AND `pattern_of` produced on the GPU, so that a caller of the two calls above stays on the device when a device of the pool fails.  Stripe b is
 * under pattern pattern_of[b] of the set of fastecc_decode_prepare_set (or FASTECC_PATTERN_NONE: a whole stripe).
 * Result: when *status == 0, every word of the pool is bit-identical to what fastecc_update_batch_set_window /
 * fastecc_update_parity_batch_set_window leave for the same list with its FASTECC_WRITE_NONE entries removed and the rows renumbered accordingly:
 * present data blocks of a touched stripe hold X' in the window, present parity blocks what fastecc_encode gives for X' in the window; absent blocks,
 * untouched stripes and words outside the window are neither read for their content nor written.  (0, block_bytes / 4) is the whole block.
 *   writes, max_per_stripe, col0_words, width_words, the rows and FASTECC_WRITE_NONE : exactly those of fastecc_update_batch_device, with its bounds of
 *             2^24 stripes and 2^24 entries.
 *   pattern_of : `count` entries of device memory, 4-byte aligned, as in fastecc_read_batch_set_device.  The host never dereferences writes,
 *             pattern_of or status: they are read when the call's kernels run, in stream order.  Entries of pattern_of for stripes that no write
 *             names are never looked at and may hold anything.
 *   max_absent : (the data form) the caller's bound on how many written data blocks are absent under their stripe's pattern.  It sizes the
 *             reconstruction buffer — min(max_absent, n_writes) rows of width_words words, owned by the context and grown on demand — and the launch
 *             that rebuilds the old rows.  0 is allowed and means the caller promises that none is absent; n_writes is always safe.  The host cannot
 *             know the number, and a buffer of n_writes blocks is 64 GiB at the call's own limits: the number is a promise, like max_per_stripe.
 *   status  : 0, or (uint32_t)code << 32 | row; the first compare-and-swap from 0 wins.  FASTECC_E_INVAL: an index >= count*k, two writes to one
 *             block, or a pattern_of[b] of a touched stripe that is neither FASTECC_PATTERN_NONE nor below the set's size.  FASTECC_E_UNSUPPORTED:
 *             a stripe with more than max_per_stripe writes.  FASTECC_E_NOMEM: more absent written blocks than max_absent; the row is one write
 *             that got no slot.  All or nothing: a non-zero status means that no word of the pool has been written by the call.
 * The return value covers what the host can decide without the lists, before any device work and with nothing written: everything
 * fastecc_update_batch_device refuses, with its codes; everything fastecc_update_batch_set_window refuses without its list (no set prepared is
 * FASTECC_E_INVAL; GF((2^61-1)^2), sharded contexts and a set "row_pitch_words" are FASTECC_E_UNSUPPORTED); FASTECC_E_INVAL for a pattern_of that
 * is null, not 4-byte aligned, or overlaps the pool, the rows, writes or status; FASTECC_E_NOMEM if the reconstruction buffer does not fit.
 * n_writes == 0 is FASTECC_OK after those checks, with *status set to 0 on the stream.
 * Streams: in steady state — the same or a smaller n_writes, count, max_per_stripe and max_absent than an earlier call on the context, and the same
 * prepared set — a call makes no host-device copy and no allocation, waits on no event or stream and uses no pinned memory.
 * fastecc_decode_prepare_set waits for a call in flight before it swaps the set's tables.  hipGraph capture is not claimed, and there are no rounds
 * beyond 16 writes per stripe.
 * Method: the three build kernels of the calls above in their set forms — the lane that opens a stripe's segment reads and
 * checks pattern_of[b], a write to an absent data block draws a row of the reconstruction buffer from one counter — then the degraded read's kernel
 * over those rows, the same parity launches with the set's table of lost parity blocks, and a scatter that leaves absent blocks alone.  Only the last
 * two write the pool, each wave behind a look at the status word.
 */
int fastecc_update_batch_set_device(fastecc_ctx *ctx, void *data, void *parity, uint64_t count, const uint32_t *pattern_of /* device, count entries */,
                                    const uint64_t *writes /* device */, uint64_t n_writes, uint32_t max_per_stripe, uint64_t max_absent,
                                    uint64_t col0_words, uint64_t width_words, const void *new_blocks, uint64_t *status /* device */, void *stream);
int fastecc_update_parity_batch_set_device(fastecc_ctx *ctx, void *parity, uint64_t count, const uint32_t *pattern_of /* device */,
                                           const uint64_t *writes /* device */, uint64_t n_writes, uint32_t max_per_stripe, uint64_t col0_words,
                                           uint64_t width_words, const void *old_blocks /* may be NULL: zero */, const void *new_blocks,
                                           uint64_t *status /* device */, void *stream);
/* Host only, no device: the code's generator-matrix entry L_i(y_q) for data block i and parity block q of the (n,k) code that
 * fastecc_create_ex(n, k, ..., flags) builds over GF(0xFFF00001), plain form in [0,p): parity block q = sum_i L_i(y_q) data block i.
 * FASTECC_E_INVAL for a null out, an index out of range or unknown flags; FASTECC_E_UNSUPPORTED for a code fastecc_create_ex refuses. */
int fastecc_code_coefficient(uint64_t n, uint64_t k, unsigned flags, uint64_t data_block, uint64_t parity_block, uint32_t *out);

/*
 * Small writes over FASTECC_FIELD_GF_P61_SQUARED: fastecc_update / fastecc_update_parity for the 64-bit field, on 16-byte elements in DEVICE
 * memory (there is no mem_kind).  fastecc_update, fastecc_update_parity and every pool form (fastecc_update_batch*, the _set and _window forms)
 * keep refusing this field with FASTECC_E_UNSUPPORTED; these two calls are the field's own, named like fastecc_gf61_binary.
 *   fastecc_gf61_update        : data is the whole k-block stripe.  Reads the old content of data[blocks[u]], adds its change to parity and
 *                                writes new_blocks[u] (count blocks, contiguous) into the stripe.
 *   fastecc_gf61_update_parity : the data blocks live elsewhere: old_blocks and new_blocks are count contiguous blocks each; old_blocks == NULL
 *                                means zero blocks (incremental encoding: zero the parity, then add blocks as they arrive).
 * Afterwards data (fastecc_gf61_update) and parity are bit for bit what fastecc_encode gives for the new stripe: canonical words, re and im < p.
 * blocks: a host array of `count` distinct indices < k in any order (it may be reused as soon as the call returns); count == 0 is a no-op and
 * there is no upper limit: a call runs in passes of at most 16 changed blocks, each one read-modify-write pass over the parity.  Enqueued on
 * `stream` without synchronising, the first call included: its weight table (72 bytes per entry, k (n/k - 1) entries for (2k,k), 4k and 8k,
 * N = 2^ceil(log2 k) entries for the other codes; 38 MB at k = 2^19) is built by a kernel on `stream` and guarded by an event of its own.
 * Inputs must be canonical (re, im < p); new_blocks / old_blocks must not overlap data or parity.
 * Codes: every code fastecc_create accepts for this field — (2k,k) with k = 2^m, 1 <= m <= 24; n = 4k and 8k; and the other (n,k) codes (zero
 * extension, fewer parity blocks), for which the update works directly on the caller's k data and n - k parity blocks: no padded copies.
 * Refusals, decided before any device work (a refused call writes nothing).  FASTECC_E_INVAL: a null context, null pointers with count > 0,
 * an index >= k, a duplicate index, pointers that are not 8-byte aligned.  FASTECC_E_UNSUPPORTED: a GF(0xFFF00001) context, a sharded
 * context, blocks of 4 GiB - 1 KiB and more (the parity kernel addresses a block through one buffer descriptor, whose range and lane offsets
 * are 32-bit byte counts).  FASTECC_E_NOMEM: the table or the 16 delta rows do not fit.
 * Cost, measured at (2^20, 2^19) x 64 KB: 13.7 ms for one changed block and 52.3 ms for 16 against 62.0 ms for a fresh
 * fastecc_encode; an update is cheaper up to 16 changed blocks (one pass) and dearer from 17 on (32: 104.8 ms).
 */
int fastecc_gf61_update(fastecc_ctx *ctx, void *data, void *parity, const uint64_t *blocks, uint64_t count, const void *new_blocks,
                        void *stream);
int fastecc_gf61_update_parity(fastecc_ctx *ctx, void *parity, const uint64_t *blocks, uint64_t count, const void *old_blocks,
                               const void *new_blocks, void *stream);
/* Host only, no device, no context: the generator-matrix entry L_i(y_q) for data block i and parity block q of the (n,k) code fastecc_create
 * builds over FASTECC_FIELD_GF_P61_SQUARED, out = (re, im), canonical: parity block q = sum_i L_i(y_q) data block i.  FASTECC_E_INVAL for
 * n <= k, data_block >= k, parity_block >= n - k or a null out; FASTECC_E_UNSUPPORTED for a shape fastecc_create refuses for this field
 * (k > 2^24; n - k above the transform order 2^ceil(log2 k) and not 3k or 7k with k a power of two). */
int fastecc_gf61_code_coefficient(uint64_t n, uint64_t k, uint64_t data_block, uint64_t parity_block, uint64_t out[2]);

/*
 * Data packing (GF.md:72-104 "Efficient data packing", README.md:160-163): RS.cpp only encodes words < p, so
 * arbitrary bytes are first recoded with one extra word per block — 4096-byte sectors become the 4100-byte
 * blocks the encoder then works on.  The reference describes this in prose and has NO code for it; the exact
 * format is therefore defined here (nothing upstream pins it):
 *   a word is (digit << 20) | low20, digit = its top 12 bits.  Only words with digit 0xFFF can be >= p.
 *   raw block   : W = block_bytes/4 - 1 arbitrary uint32 words (1 <= W <= 1024)
 *   packed block: W + 1 words, all < 0xFFF00000 < p.  Word j keeps low20 of raw word j; the digit string is
 *     flag word (word W) = 0 : no raw digit is 0xFFF, digits unchanged;
 *     flag word          = 1 : [one 11-bit entry per 0xFFF digit, in increasing position: position | 0x400 if
 *                               another entry follows][all other digits in their original order].
 * The context must be GF(0xFFF00001) with block_bytes = 4 * (W + 1) (e.g. 4100); raw stripes are k * 4W bytes,
 * packed stripes k * block_bytes bytes, both block-major and contiguous — except that DEVICE packed stripes use
 * the context's "row_pitch_words" option like fastecc_encode does (e.g. 1056: rows padded to 4224 bytes, which
 * is what makes 4100-byte blocks encode at full speed).  DEVICE pointers: enqueued on `stream`.
 * fastecc_unpack_blocks also validates: a block no packer produces (flag > 1, a 0xFFF digit left, entries not
 * strictly increasing / out of range / never ending) is copied through unchanged and counted in *bad_blocks
 * (may be NULL = not wanted; non-NULL makes the call synchronise `stream`).
 */
int fastecc_pack_blocks(fastecc_ctx *ctx, const void *raw, void *packed, int mem_kind, void *stream);
int fastecc_unpack_blocks(fastecc_ctx *ctx, const void *packed, void *raw, int mem_kind, void *stream, uint64_t *bad_blocks);

/* Host-side field helpers (GF(p).cpp:254-297), used to build tables and by bindings. */
uint32_t fastecc_gf_mul(uint32_t x, uint32_t y);
uint32_t fastecc_gf_pow(uint32_t x, uint32_t e);
uint32_t fastecc_gf_root(uint32_t order); /* 19^((p-1)/order); order must divide 2^20 */
uint32_t fastecc_gf_inv(uint32_t x);
/* Berlekamp-Massey over GF(0xFFF00001): the shortest LFSR that generates the `count` syndromes s (reduced mod p) — for power
 * sums s_i = sum Y X^i the error locator Lambda(x) = prod (1 - X x).  Writes Lambda_0 = 1 .. Lambda_L to lambda and returns L;
 * FASTECC_E_INVAL for a null pointer or cap < L + 1.  Host only (used by fastecc_locate_errors). */
int fastecc_gf_berlekamp_massey(const uint32_t *s, uint32_t count, uint32_t *lambda, uint32_t cap);
/* The same for FASTECC_FIELD_GF_P61_SQUARED: z[0] = re, z[1] = im (inputs are reduced mod p); out may alias.
 * fastecc_gf61_root returns FASTECC_E_INVAL unless order is a power of two <= 2^62. */
int fastecc_gf61_mul(const uint64_t x[2], const uint64_t y[2], uint64_t out[2]);
int fastecc_gf61_pow(const uint64_t x[2], uint64_t e, uint64_t out[2]);
int fastecc_gf61_inv(const uint64_t x[2], uint64_t out[2]);
int fastecc_gf61_root(uint64_t order, uint64_t out[2]);

/*
 * Introspection for the benchmark: time the last `fastecc_encode` enqueued on DEVICE memory spent in
 * kernels, measured with HIP events on the stream it ran on.  Enable before the encode calls.
 *   fastecc_profile_enable(ctx, 1)  -> every kernel launch is bracketed by hipEvents
 *   fastecc_profile_read(ctx, names, ms, launches, cap) -> per-kernel accumulated ms and launch counts
 *                                      since the last reset (synchronises the stream); returns the
 *                                      number of distinct kernels written (<= cap)
 */
int fastecc_profile_enable(fastecc_ctx *ctx, int on);
int fastecc_profile_read(fastecc_ctx *ctx, const char **names, double *ms, uint64_t *launches, int cap);
/* As above, plus the accumulated ALGORITHMIC bytes of those launches (each launch reads its part of the stripe
 * once and writes it once): bytes[i] / launches[i] is the per-launch figure the roofline uses. */
int fastecc_profile_read_bytes(fastecc_ctx *ctx, const char **names, double *ms, uint64_t *launches, uint64_t *bytes, int cap);
int fastecc_profile_reset(fastecc_ctx *ctx);

/* Plan description, e.g. "dif5,dif5,...|mid...|dit..." — for logs and DESIGN.md tables. */
const char *fastecc_plan_string(fastecc_ctx *ctx);
/*
 * Tuning options (all bit-exact; defaults are the measured best on MI355X).
 *   "cache_policy" 0..15: bit 0/1 non-temporal stripe loads/stores in the outer passes, bit 2/3 in MID (default 15);
 *   "xcd_swizzle"  0..2 : tile order per XCD (default 1);
 *   "row_pitch_words" = L >= block_bytes/4 (0 = contiguous): DEVICE stripes given to fastecc_encode are [k][L]
 *                  words, the first block_bytes/4 of each row valid, the rest untouched.  Lets a host that owns its
 *                  HBM layout pad odd block sizes (2052, 4100 bytes) to a multiple of 128 bytes: +50 % throughput.
 *                  fastecc_pack_blocks / _unpack_blocks follow the pitch on their packed side; the other entry
 *                  points return FASTECC_E_UNSUPPORTED while a pitch is set;
 *   "host_slabs" = 1 .. 32, a power of two (default 8): column slabs of the FASTECC_MEM_HOST_PINNED pipeline (and of the FASTECC_MEM_HOST one);
 *   "stage_threads" = 0 .. 64 (default 0 = min(6, hardware threads / 4)): helper threads per staging ring (pageable host memory: FASTECC_MEM_HOST
 *                  results, fastecc_encode_blocks); 4 to 12 measured the same on a 16-CPU share (profiles/r04/encode_blocks_bench.jsonl);
 *   "host_pipeline" = 0 / 1 (default 0): 1 = FASTECC_MEM_HOST encodes of (2k,k) stripes of 256 MiB and more move pageable memory through two
 *                  rings of pinned slots (64 MiB each, allocated at the first such call) served by helper threads, slab h going up while
 *                  slab h - 1 comes down; 0 = upload, encode, download one after the other (the download still through its ring).  The
 *                  pipeline is bounded by what the host's cores copy, not by the link: 65-100 ms against 81-97 (by box) for 2 + 2 GiB in
 *                  a 16-CPU share of an EPYC 9575F (profiles/r04/host_pageable_pipeline.jsonl) — worth it on a host with cores to spare;
 *   "encode_direct_max" = 0..256 (default 160): codes with at most this many parity blocks (n - k) are encoded straight from the Lagrange
 *                  basis — one read of the data (0.4 ms up to 16 parity blocks ... 1.4 ms for 128 at k = 2^19 x 4 KB) instead of the transform
 *                  pipeline (2.4 ms); same parity bits.  Rows the matrix-core kernel cannot take (odd length, < 64 words, not 8-byte aligned)
 *                  stop at 32;
 *   "decode_direct_max" = 0..256 (default 256; 0..32 for GF((2^61-1)^2)): lost blocks up to which the decoder's direct path is used (next
 *                  decode_prepare); rows the matrix-core kernel cannot take stop at 96 (not for mixed-radix orders above 2^20, whose transform
 *                  path is much dearer: there the option alone decides);
 *   "locate_max" = 0..4096 (default 256): the most unknown corrupted blocks fastecc_locate_errors / fastecc_correct look for;
 *   "decode_split" = 0 / 1 / 2 (default 1; codes over GF(0xFFF00001) with n <= 2k and k >= 2^17 (power-of-two orders), next decode_prepare): the
 *                  decoder's 2k-point transform as two transforms of k points — the data half, and of the parity half only the blocks needed: the
 *                  survivors at multiples of 2^h of that half (largest h <= 5 that leaves as many as there are lost data blocks), whose transform is
 *                  one of k >> h rows (2 % of the codeword lost: decode 7.1 -> 3.8 ms at k = 2^19 x 4 KB), else the surviving blocks of the first
 *                  few block groups (what round 3 always did: 2 = that form only); 0 = one transform of 2k points.  Same bits.
 *                  GF((2^61-1)^2), k >= 2^11: 0 / 1 (default 1) — the same split in its k >> h form (h = 5 .. 1): decode 7.2 -> 4.5 ms, repair 9.2 -> 6.8 ms (a second MID + DIT chain for the lost parity blocks) at
 *                  k = 2^19 x 4 KB and 2 % lost, 72 ms = 1.14 x the encode at 64 KB blocks; patterns it does not take run the folded 2k-point transform;
 *   "direct_kernel" = 0 / 1 / 2 (default 0 = choose): the kernel of those direct paths — 1 = VALU (96-bit lazy accumulation, any rows),
 *                  2 = MFMA (i8 digits; falls back to 1 where it cannot run).  Same bits either way;
 *   "decode_batch_kernel" = 0 / 1 / 2 (default 0 = choose; at call time): how fastecc_decode_batch / _repair_batch run a direct-path pass — 1 = one
 *                  launch over all stripes whenever the pass allows it, 2 = stripe by stripe (direct_kernel then picks the kernel).  Same bits either way.
 *                  fastecc_decode_batch_set / _repair_batch_set read it too: 0 = one launch per class unless its passes read 4096 blocks or more,
 *                  1 = one launch per class always, 2 = stripe by stripe;
 *   "encode_pool_kernel" = 0 / 1 / 2 / 3 (default 0 = choose; at call time): how fastecc_encode_pool runs a code of the direct path — 1 = the VALU
 *                  batch kernel (96-bit lazy accumulation; any block size and alignment), 2 = the matrix-core pool kernel (i8 digits, a wave per stripe
 *                  and 64 words; needs an even block of at least 64 words, 8-byte aligned pools, k < 4096 and a stripe below 4 GiB, and falls back
 *                  to 1 where it cannot run), 3 = stripe by stripe (also for the (2k,k) codes of the transform path); 0 = one launch when k < 4096
 *                  and it fills at least 1024 waves (the matrix-core kernel from n - k = 4 on where it can run: measured 1.1 x the VALU kernel at (20,16), 1.8 x at (48,32)), else stripe by stripe.  Same bits in every mode;
 *   "scrub_batch_chunk" = 0 .. INT_MAX (default 0 = the context's chunk capacity; at call time): the most stripes per chunk of
 *                  fastecc_verify_batch / _correct_batch / _locate_errors_batch.  Same answers either way;
 *   "correct_batch_mode" = 0 / 1 / 2 (default 0 = choose; at call time): how fastecc_correct_batch and fastecc_correct_batch_set correct the inconsistent stripes — 1 = batched
 *                  location and one repair per lost-block pattern for every stripe that qualifies, 2 = fastecc_correct stripe by stripe, 0 = 1 when
 *                  at least two inconsistent stripes qualify, else 2.  Same status and same bytes either way;
 *   "fuse_radix" = 0 / 1 (default 1; mixed-radix contexts): the odd-radix level fused into the outer tile passes, or as its own passes;
 *   "slabs" = H (1..32): encode H column slabs of the stripe on internal streams, each one pass
 * behind the previous, so that different kinds of passes overlap on the GPU, or with "slab_mode" = 1 one
 * after the other on `stream` (a memory-side-cache experiment: profiles/r02/slab_cache_sweep.md — neither pays).  The call
 * still behaves as one operation on `stream`: it starts after prior work on `stream` and later work on `stream` waits for it.
 */
int fastecc_set_option(fastecc_ctx *ctx, const char *name, int value);

/* Select the kernel plan (0 = default).  Exposed so bench.py can A/B plans; see DESIGN.md §5.  3100 is the split of rounds 1-4 (dif9 / mid10 / dit9
 * at k = 2^19); the default gives MID one level fewer for the power-of-two codes from k = 2^16 up (3090: dif10 / mid9 / dit10; 4090 at 2^18:
 * outer tiles of 64-word rows).  Every plan computes the same words. */
int fastecc_set_plan(fastecc_ctx *ctx, int plan);

/*
 * Host-only introspection (no HIP device is touched): the pass plan that (k, block_bytes, plan) selects,
 * and the level-packed twiddle table that goes with it — what replaces the roots[] array of
 * ntt.cpp:397-402.  which: 0 = encode/interpolate (inverse roots), 1 = encode/evaluate (forward roots),
 * 2 = fastecc_ntt forward, 3 = fastecc_ntt inverse.  `out` receives k words (Montgomery form, w*2^32 mod p;
 * level l at [2^l, 2^(l+1))); level_stride (optional, log2(k) ints) the log2 stride of the register run
 * that executes each level.
 */
int fastecc_plan_describe(uint64_t k, uint64_t block_bytes, int plan, char *buf, size_t cap);
int fastecc_plan_twiddles(uint64_t k, uint64_t block_bytes, int plan, int which, uint32_t *out, int32_t *level_stride);

#ifdef __cplusplus
}
#endif
#endif /* FASTECC_H */
