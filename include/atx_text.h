/*
 * atx_text.h — C ABI of libatx_text, the text-column kernels that go with libatx (MI355X, gfx950).
 *
 * A companion library with its own header: libatx's entry points are a fixed set
 * (include/atx.h, ATX_VERSION 420) typed for numeric columns, and a byte matrix
 * is a different kind of argument.  The two libraries share no symbol and no
 * state; this header includes atx.h only for the status codes (ATX_OK,
 * ATX_EINVAL, ATX_EHIP, ...), which mean here what they mean there.
 *
 * Conventions (atx.h states them in full; they hold unchanged)
 *  - Plain C types only.  Every pointer named in a signature is a DEVICE pointer
 *    (HBM).  The caller owns every buffer; the library allocates nothing and
 *    keeps no state besides a thread-local error string.  A buffer of ZERO
 *    elements may be NULL: the call validates the rest, launches nothing and
 *    returns ATX_OK.
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Calls
 *    enqueue work and return without synchronising.
 *  - Return value: ATX_OK (0) or a negative ATX_E* code; atx_text_last_error()
 *    gives the message for the calling thread.  Nothing throws across the ABI.
 *  - Every entry point is re-entrant.
 *
 * A *text column* of n rows is a row-major [n, width] matrix of bytes with a row
 * pitch in bytes (pitch >= width): row r holds the UTF-8 bytes of its string at
 * text[r * pitch .. r * pitch + width), zero-padded on the right.  The bytes
 * between width and pitch are never read.
 */
#ifndef ATX_TEXT_H
#define ATX_TEXT_H

#include <stddef.h>
#include <stdint.h>

#include "atx.h"

/* Built with -fvisibility=hidden and a version script made from this header: the ATX_TEXT_API declarations below are the library's
 * ONLY dynamic symbols (tests/test_statids_host.py checks `nm -D --defined-only` against this header). */
#if defined(_WIN32)
#define ATX_TEXT_API
#else
#define ATX_TEXT_API __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define ATX_TEXT_VERSION 420  /* goes with ATX_VERSION */
#define ATX_TEXT_MAX_WIDTH 256 /* bytes per row: bounds the per-lane loops (five MD5 blocks at most) */

/* ATX_TEXT_VERSION of the library that was loaded. */
ATX_TEXT_API int atx_text_version(void);

/* The message of the last failed call of the calling thread ("" if none); valid until that thread's next failing call. */
ATX_TEXT_API const char* atx_text_last_error(void);

/*
 * Station identifiers as integers, one row per lane, one launch per column.
 * R: filters/tabular/encode_statids.py:45-57 — s = id.strip().upper(); int(s, 36) where s is non-empty and all of its characters are
 * in 0-9A-Z, else the first four bytes of md5(id.strip().encode()) read little-endian, unsigned — restricted to ASCII:
 *
 *   end        one past the last non-zero byte of the row.
 *   undecided  a byte >= 0x80 anywhere in the row, or a zero byte before `end`: code = 0, undecided = 1, and the caller evaluates the
 *              reference's statement itself (Python's Unicode strip() and upper() are not attempted).
 *   strip      both ends lose the bytes 0x09-0x0D, 0x1C-0x1F and 0x20 (what str.strip() strips below 0x80); interior ones stay.
 *   base 36    the stripped string is non-empty and every byte, a-z read as A-Z, is in 0-9A-Z.  Up to 12 characters: code is the
 *              base-36 value (36^12 - 1 < 2^63, exact); 13 or more: undecided (the value may not fit an int64).
 *   md5        anything else, the empty string included: code = bytes 0 .. 3 of the RFC 1321 digest of the stripped bytes (NOT
 *              upper-cased), little-endian, as an unsigned 32-bit value.  Any stripped length up to `width` (one to five blocks).
 *
 * text: uint8 [n, pitch]; width in 1 .. ATX_TEXT_MAX_WIDTH; pitch >= width, in bytes.  code: int64 [n]; undecided: uint8 [n] (0 or 1).
 * Rows are indexed in 64 bits.  A 4-byte-aligned `text` with a pitch that is a multiple of 4 is read in dwords, anything else bytewise;
 * the results are the same.
 * ATX_EINVAL: n < 0, width outside 1 .. ATX_TEXT_MAX_WIDTH, pitch < width, or a NULL pointer with n > 0 — nothing is launched.
 * n == 0: ATX_OK, nothing launched, the pointers may be NULL.
 */
ATX_TEXT_API int atx_text_encode_statids(const uint8_t* text, int64_t n, int32_t width, int64_t pitch, int64_t* code, uint8_t* undecided,
                                         void* stream);

#ifdef __cplusplus
}
#endif

#endif /* ATX_TEXT_H */
