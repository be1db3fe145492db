// Station identifiers as integers: atx_text_encode_statids (include/atx_text.h).  One row of a byte matrix per lane.
//
// The reference's encode_statids filter applies a Python callable to every row (R: filters/tabular/encode_statids.py:45-57):
//     s = id.strip().upper();  int(s, 36) if s and all(c in "0-9A-Z" for c in s) else int.from_bytes(md5(id.strip().encode())[:4], "little")
// Here that is integer work per row on the UTF-8 bytes, for the rows whose bytes are all ASCII; a row with a byte >= 0x80, a zero byte
// before its last non-zero byte, or 13 and more base-36 characters (the value may pass 2^63) is flagged `undecided` and left to the
// caller, which evaluates the statement itself.  tests/statids_restatement.py holds the same rules in Python and numpy.
//
// One pass over the row finds, byte by byte: `end` (one past the last non-zero byte) and the count of non-zero bytes (they differ where
// a zero lies inside), the high-bit flag, the stripped range [start, stop) — Python's ASCII whitespace is 0x09-0x0D, 0x1C-0x1F, 0x20 —
// and, alongside, the base-36 value, the count of characters and whether all of them were digits: whitespace after the first
// character is only `pending` until another character follows it, which makes it interior and the string no number.  The accumulator
// may wrap beyond 12 characters; such a row is undecided and the value is not used.
//
// Rows that are no number take MD5 (RFC 1321) over bytes [start, stop): (L + 8) / 64 + 1 blocks, at most five for 256 bytes.  The
// sixteen message words of a block are sixteen named registers, each built by a function of a compile-time offset within the block —
// a whole dword where the message covers it, else byte by byte with the 0x80 terminator and zeros, the bit length in words 14 and
// 15 of the last block — and the 64 rounds are unrolled with their message index, rotation and constant as literals, so nothing is
// indexed at run time and the kernel needs no scratch memory (tools/kernel_resources.py --lib lib/libatx_text.so;
// profiles/statids_resources.json).  A wave in which no row needs MD5 skips it.
//
// Launch shape, as atx_obs_rowset.hip: one row per lane, 256-lane workgroups, a grid-stride loop under a grid cap, 64-bit row
// indices.  A row of `pitch` bytes per lane coalesces when the pitch is small and a multiple of 4: the DWORDS instance (4-byte-aligned
// base, pitch % 4 == 0) reads the whole dwords of a row as dwords and the last width % 4 bytes singly; the other reads bytes.  Neither
// reads a byte at or beyond `width`.  No floating point, no LDS, no atomics; plain vector stores.
#include <cstring>

#include "../../../include/atx_text.h"
#include "../atx_host.hpp"

namespace atx_text {

constexpr int kBlock = 256;  // 4 waves: one per SIMD of a CU
constexpr int kGrid = 2048;  // grid cap, as kRsGrid: beyond 2^19 rows a lane takes further rows

// ---- the scan of one row ---------------------------------------------------------------------------------------------------------------
struct Scan {
    uint32_t end = 0, nonzero = 0;    // one past the last non-zero byte; how many bytes are non-zero
    uint32_t start = 0, stop = 0;     // the stripped string
    uint32_t n_char = 0;              // stop - start wherever `digits` still holds
    uint64_t value = 0;               // base 36, modulo 2^64
    bool high = false, found = false, pending = false, digits = true;
};

__host__ __device__ __forceinline__ void scan_byte(Scan& s, uint32_t b, uint32_t pos) {
    const bool space = (b - 0x09u <= 0x04u) || (b - 0x1cu <= 0x04u);  // 0x09-0x0D, 0x1C-0x20
    s.high |= b >= 0x80u;
    if (b != 0) {
        s.end = pos + 1;
        ++s.nonzero;
    }
    if (b != 0 && !space) {
        if (!s.found) s.start = pos;
        s.found = true;
        s.stop = pos + 1;
        if (s.pending) s.digits = false;  // whitespace inside the string
        uint32_t d = b - (uint32_t)'0';
        if (d > 9u) {
            d = (b | 0x20u) - (uint32_t)'a' + 10u;
            if (d - 10u > 25u) s.digits = false;
        }
        s.value = s.value * 36u + d;
        ++s.n_char;
    } else if (space && s.found) {
        s.pending = true;
    }
}

template <bool DWORDS>
__host__ __device__ __forceinline__ Scan scan_row(const uint8_t* __restrict__ row, uint32_t width) {
    Scan s;
    uint32_t pos = 0;
    if constexpr (DWORDS) {
        const uint32_t* __restrict__ words = reinterpret_cast<const uint32_t*>(row);
        for (; pos + 4 <= width; pos += 4) {
            const uint32_t w = words[pos >> 2];
            scan_byte(s, w & 0xffu, pos);
            scan_byte(s, (w >> 8) & 0xffu, pos + 1);
            scan_byte(s, (w >> 16) & 0xffu, pos + 2);
            scan_byte(s, w >> 24, pos + 3);
        }
    }
    for (; pos < width; ++pos) scan_byte(s, row[pos], pos);
    return s;
}

// ---- MD5 -------------------------------------------------------------------------------------------------------------------------------
// Message word at byte offset `off` of the padded message: text[0 .. L), 0x80, zeros.  (The length words are set by the caller.)
__host__ __device__ __forceinline__ uint32_t message_word(const uint8_t* __restrict__ text, uint32_t L, uint32_t off) {
    if (off > L) return 0u;
    uint32_t w = 0u;
    if (off + 4u <= L) {
        memcpy(&w, text + off, 4);  // any alignment: the stripped string starts where it starts
        return w;
    }
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) {
        const uint32_t p = off + i;
        if (p < L) w |= (uint32_t)text[p] << (8 * i);
        else if (p == L) w |= 0x80u << (8 * i);
    }
    return w;
}

__host__ __device__ __forceinline__ uint32_t rotl(uint32_t x, int s) { return (x << s) | (x >> (32 - s)); }

// One round: I, the message word M, the rotation S and the constant K are literals at every use.
#define ATX_MD5_F(b, c, d) (((b) & (c)) | (~(b) & (d)))
#define ATX_MD5_G(b, c, d) (((d) & (b)) | (~(d) & (c)))
#define ATX_MD5_H(b, c, d) ((b) ^ (c) ^ (d))
#define ATX_MD5_I(b, c, d) ((c) ^ ((b) | ~(d)))
#define ATX_MD5_STEP(FN, a, b, c, d, M, K, S) (a) = (b) + rotl((a) + FN(b, c, d) + (M) + (K), (S))

// The first 32 bits of the state after the last block: bytes 0 .. 3 of the digest, little-endian.
__host__ __device__ __forceinline__ uint32_t md5_first_word(const uint8_t* __restrict__ text, uint32_t L) {
    uint32_t A = 0x67452301u, B = 0xefcdab89u, C = 0x98badcfeu, D = 0x10325476u;
    const uint32_t n_blocks = (L + 8u) / 64u + 1u;
    for (uint32_t blk = 0; blk < n_blocks; ++blk) {
        const uint32_t base = blk * 64u;
        const bool last = blk + 1u == n_blocks;
        const uint32_t m0 = message_word(text, L, base + 0u), m1 = message_word(text, L, base + 4u);
        const uint32_t m2 = message_word(text, L, base + 8u), m3 = message_word(text, L, base + 12u);
        const uint32_t m4 = message_word(text, L, base + 16u), m5 = message_word(text, L, base + 20u);
        const uint32_t m6 = message_word(text, L, base + 24u), m7 = message_word(text, L, base + 28u);
        const uint32_t m8 = message_word(text, L, base + 32u), m9 = message_word(text, L, base + 36u);
        const uint32_t m10 = message_word(text, L, base + 40u), m11 = message_word(text, L, base + 44u);
        const uint32_t m12 = message_word(text, L, base + 48u), m13 = message_word(text, L, base + 52u);
        const uint32_t m14 = last ? L * 8u : message_word(text, L, base + 56u);  // the length in BITS, 64 bits little-endian
        const uint32_t m15 = last ? 0u : message_word(text, L, base + 60u);
        uint32_t a = A, b = B, c = C, d = D;
        ATX_MD5_STEP(ATX_MD5_F, a, b, c, d, m0, 0xd76aa478u, 7);
        ATX_MD5_STEP(ATX_MD5_F, d, a, b, c, m1, 0xe8c7b756u, 12);
        ATX_MD5_STEP(ATX_MD5_F, c, d, a, b, m2, 0x242070dbu, 17);
        ATX_MD5_STEP(ATX_MD5_F, b, c, d, a, m3, 0xc1bdceeeu, 22);
        ATX_MD5_STEP(ATX_MD5_F, a, b, c, d, m4, 0xf57c0fafu, 7);
        ATX_MD5_STEP(ATX_MD5_F, d, a, b, c, m5, 0x4787c62au, 12);
        ATX_MD5_STEP(ATX_MD5_F, c, d, a, b, m6, 0xa8304613u, 17);
        ATX_MD5_STEP(ATX_MD5_F, b, c, d, a, m7, 0xfd469501u, 22);
        ATX_MD5_STEP(ATX_MD5_F, a, b, c, d, m8, 0x698098d8u, 7);
        ATX_MD5_STEP(ATX_MD5_F, d, a, b, c, m9, 0x8b44f7afu, 12);
        ATX_MD5_STEP(ATX_MD5_F, c, d, a, b, m10, 0xffff5bb1u, 17);
        ATX_MD5_STEP(ATX_MD5_F, b, c, d, a, m11, 0x895cd7beu, 22);
        ATX_MD5_STEP(ATX_MD5_F, a, b, c, d, m12, 0x6b901122u, 7);
        ATX_MD5_STEP(ATX_MD5_F, d, a, b, c, m13, 0xfd987193u, 12);
        ATX_MD5_STEP(ATX_MD5_F, c, d, a, b, m14, 0xa679438eu, 17);
        ATX_MD5_STEP(ATX_MD5_F, b, c, d, a, m15, 0x49b40821u, 22);

        ATX_MD5_STEP(ATX_MD5_G, a, b, c, d, m1, 0xf61e2562u, 5);
        ATX_MD5_STEP(ATX_MD5_G, d, a, b, c, m6, 0xc040b340u, 9);
        ATX_MD5_STEP(ATX_MD5_G, c, d, a, b, m11, 0x265e5a51u, 14);
        ATX_MD5_STEP(ATX_MD5_G, b, c, d, a, m0, 0xe9b6c7aau, 20);
        ATX_MD5_STEP(ATX_MD5_G, a, b, c, d, m5, 0xd62f105du, 5);
        ATX_MD5_STEP(ATX_MD5_G, d, a, b, c, m10, 0x02441453u, 9);
        ATX_MD5_STEP(ATX_MD5_G, c, d, a, b, m15, 0xd8a1e681u, 14);
        ATX_MD5_STEP(ATX_MD5_G, b, c, d, a, m4, 0xe7d3fbc8u, 20);
        ATX_MD5_STEP(ATX_MD5_G, a, b, c, d, m9, 0x21e1cde6u, 5);
        ATX_MD5_STEP(ATX_MD5_G, d, a, b, c, m14, 0xc33707d6u, 9);
        ATX_MD5_STEP(ATX_MD5_G, c, d, a, b, m3, 0xf4d50d87u, 14);
        ATX_MD5_STEP(ATX_MD5_G, b, c, d, a, m8, 0x455a14edu, 20);
        ATX_MD5_STEP(ATX_MD5_G, a, b, c, d, m13, 0xa9e3e905u, 5);
        ATX_MD5_STEP(ATX_MD5_G, d, a, b, c, m2, 0xfcefa3f8u, 9);
        ATX_MD5_STEP(ATX_MD5_G, c, d, a, b, m7, 0x676f02d9u, 14);
        ATX_MD5_STEP(ATX_MD5_G, b, c, d, a, m12, 0x8d2a4c8au, 20);

        ATX_MD5_STEP(ATX_MD5_H, a, b, c, d, m5, 0xfffa3942u, 4);
        ATX_MD5_STEP(ATX_MD5_H, d, a, b, c, m8, 0x8771f681u, 11);
        ATX_MD5_STEP(ATX_MD5_H, c, d, a, b, m11, 0x6d9d6122u, 16);
        ATX_MD5_STEP(ATX_MD5_H, b, c, d, a, m14, 0xfde5380cu, 23);
        ATX_MD5_STEP(ATX_MD5_H, a, b, c, d, m1, 0xa4beea44u, 4);
        ATX_MD5_STEP(ATX_MD5_H, d, a, b, c, m4, 0x4bdecfa9u, 11);
        ATX_MD5_STEP(ATX_MD5_H, c, d, a, b, m7, 0xf6bb4b60u, 16);
        ATX_MD5_STEP(ATX_MD5_H, b, c, d, a, m10, 0xbebfbc70u, 23);
        ATX_MD5_STEP(ATX_MD5_H, a, b, c, d, m13, 0x289b7ec6u, 4);
        ATX_MD5_STEP(ATX_MD5_H, d, a, b, c, m0, 0xeaa127fau, 11);
        ATX_MD5_STEP(ATX_MD5_H, c, d, a, b, m3, 0xd4ef3085u, 16);
        ATX_MD5_STEP(ATX_MD5_H, b, c, d, a, m6, 0x04881d05u, 23);
        ATX_MD5_STEP(ATX_MD5_H, a, b, c, d, m9, 0xd9d4d039u, 4);
        ATX_MD5_STEP(ATX_MD5_H, d, a, b, c, m12, 0xe6db99e5u, 11);
        ATX_MD5_STEP(ATX_MD5_H, c, d, a, b, m15, 0x1fa27cf8u, 16);
        ATX_MD5_STEP(ATX_MD5_H, b, c, d, a, m2, 0xc4ac5665u, 23);

        ATX_MD5_STEP(ATX_MD5_I, a, b, c, d, m0, 0xf4292244u, 6);
        ATX_MD5_STEP(ATX_MD5_I, d, a, b, c, m7, 0x432aff97u, 10);
        ATX_MD5_STEP(ATX_MD5_I, c, d, a, b, m14, 0xab9423a7u, 15);
        ATX_MD5_STEP(ATX_MD5_I, b, c, d, a, m5, 0xfc93a039u, 21);
        ATX_MD5_STEP(ATX_MD5_I, a, b, c, d, m12, 0x655b59c3u, 6);
        ATX_MD5_STEP(ATX_MD5_I, d, a, b, c, m3, 0x8f0ccc92u, 10);
        ATX_MD5_STEP(ATX_MD5_I, c, d, a, b, m10, 0xffeff47du, 15);
        ATX_MD5_STEP(ATX_MD5_I, b, c, d, a, m1, 0x85845dd1u, 21);
        ATX_MD5_STEP(ATX_MD5_I, a, b, c, d, m8, 0x6fa87e4fu, 6);
        ATX_MD5_STEP(ATX_MD5_I, d, a, b, c, m15, 0xfe2ce6e0u, 10);
        ATX_MD5_STEP(ATX_MD5_I, c, d, a, b, m6, 0xa3014314u, 15);
        ATX_MD5_STEP(ATX_MD5_I, b, c, d, a, m13, 0x4e0811a1u, 21);
        ATX_MD5_STEP(ATX_MD5_I, a, b, c, d, m4, 0xf7537e82u, 6);
        ATX_MD5_STEP(ATX_MD5_I, d, a, b, c, m11, 0xbd3af235u, 10);
        ATX_MD5_STEP(ATX_MD5_I, c, d, a, b, m2, 0x2ad7d2bbu, 15);
        ATX_MD5_STEP(ATX_MD5_I, b, c, d, a, m9, 0xeb86d391u, 21);
        A += a;
        B += b;
        C += c;
        D += d;
    }
    return A;
}

// ---- one row ---------------------------------------------------------------------------------------------------------------------------
template <bool DWORDS>
__host__ __device__ __forceinline__ void encode_row(const uint8_t* __restrict__ row, uint32_t width, int64_t* code, uint8_t* undecided) {
    const Scan s = scan_row<DWORDS>(row, width);
    const bool number = s.found && s.digits;
    if (s.high || s.nonzero != s.end || (number && s.n_char > 12u)) {
        *code = 0;
        *undecided = 1;
        return;
    }
    *undecided = 0;
    *code = number ? (int64_t)s.value : (int64_t)md5_first_word(row + s.start, s.stop - s.start);
}

template <bool DWORDS>
__global__ __launch_bounds__(kBlock) void text_statids_kernel(const uint8_t* __restrict__ text, int64_t n, uint32_t width, int64_t pitch,
                                                              int64_t* __restrict__ code, uint8_t* __restrict__ undecided) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < n; r += stride) {
        int64_t c;
        uint8_t u;
        encode_row<DWORDS>(text + r * pitch, width, &c, &u);
        code[r] = c;
        undecided[r] = u;
    }
}

}  // namespace atx_text

extern "C" int atx_text_version(void) { return ATX_TEXT_VERSION; }

extern "C" const char* atx_text_last_error(void) { return atx::last_error().c_str(); }

extern "C" int atx_text_encode_statids(const uint8_t* text, int64_t n, int32_t width, int64_t pitch, int64_t* code, uint8_t* undecided,
                                       void* stream) {
    using namespace atx_text;
    ATX_REQUIRE(n >= 0, ATX_EINVAL, "atx_text_encode_statids: n = %lld is negative", (long long)n);
    ATX_REQUIRE(width >= 1 && width <= ATX_TEXT_MAX_WIDTH, ATX_EINVAL, "atx_text_encode_statids: width = %d is outside 1 .. %d", (int)width,
                ATX_TEXT_MAX_WIDTH);
    ATX_REQUIRE(pitch >= width, ATX_EINVAL, "atx_text_encode_statids: pitch = %lld is below width = %d", (long long)pitch, (int)width);
    if (n == 0) return ATX_OK;
    ATX_REQUIRE(text && code && undecided, ATX_EINVAL, "atx_text_encode_statids: null pointer (text=%p code=%p undecided=%p) with n = %lld",
                (const void*)text, (void*)code, (void*)undecided, (long long)n);
    const unsigned grid = atx::grid_for(n, kBlock, kGrid);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if ((reinterpret_cast<uintptr_t>(text) & 3u) == 0 && (pitch & 3) == 0)
        hipLaunchKernelGGL(text_statids_kernel<true>, dim3(grid), dim3(kBlock), 0, s, text, n, (uint32_t)width, pitch, code, undecided);
    else
        hipLaunchKernelGGL(text_statids_kernel<false>, dim3(grid), dim3(kBlock), 0, s, text, n, (uint32_t)width, pitch, code, undecided);
    ATX_LAUNCH_CHECK("atx_text_encode_statids");
    return ATX_OK;
}
