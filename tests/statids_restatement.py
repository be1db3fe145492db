"""encode_statids in this project's own words, with one-at-a-time defects, and the kernel's byte-level rules in numpy.

``statid_to_int`` is the statement of the reference's filter (R: filters/tabular/encode_statids.py:45-57): strip, upper-case, and the
base-36 value if the string is non-empty and made of ``0-9A-Z`` only, else the first four bytes of the MD5 digest of the stripped
(not upper-cased) string, little-endian.  ``defect=`` switches on ONE wrong variant, each a mistake a kernel could make; the golden
edge table (tests/golden/statids.json) must catch every one of them (tests/test_statids_host.py).

``pack`` lays strings out as the kernel reads them — a ``[n, pitch]`` byte matrix, UTF-8, zero-padded — and ``kernel_rules`` predicts
from those bytes alone which rows the kernel leaves undecided: a byte >= 0x80, a zero byte before the last non-zero byte, or 13 and
more base-36 characters after the ASCII strip.  ``expected`` joins the two: the codes and flags a launch must return.
"""

from __future__ import annotations

import hashlib
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "statids.json")
DIGITS = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ"
ASCII_SPACE = bytes([0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x1C, 0x1D, 0x1E, 0x1F, 0x20])  # what str.strip() strips below 0x80
DEFECTS = ("upper_before_md5", "no_strip_1c_1f", "strip_interior", "digest_big_endian", "pad_single_block_only",
           "length_in_bytes_not_bits", "wrap_13_chars", "empty_is_zero")
MAX_WIDTH = 256  # ATX_TEXT_MAX_WIDTH


# ---- MD5 written out (RFC 1321), so that its padding rules can be broken on purpose ----------------------------------------------------
_S = [7, 12, 17, 22] * 4 + [5, 9, 14, 20] * 4 + [4, 11, 16, 23] * 4 + [6, 10, 15, 21] * 4
_K = [int(abs(__import__("math").sin(i + 1)) * 2**32) & 0xFFFFFFFF for i in range(64)]


def md5_digest(message: bytes, *, single_block: bool = False, length_in_bytes: bool = False) -> bytes:
    length = len(message) if length_in_bytes else 8 * len(message)
    if single_block:  # the padding of a message that fits one block, applied to any: the length words overwrite bytes 56 .. 63
        block = bytearray((message + b"\x80" + bytes(64))[:64])
        block[56:64] = (length & (2**64 - 1)).to_bytes(8, "little")
        padded = bytes(block)
    else:
        padded = message + b"\x80" + bytes((55 - len(message)) % 64) + (length & (2**64 - 1)).to_bytes(8, "little")
    state = [0x67452301, 0xEFCDAB89, 0x98BADCFE, 0x10325476]
    for at in range(0, len(padded), 64):
        m = [int.from_bytes(padded[at + 4 * k:at + 4 * k + 4], "little") for k in range(16)]
        a, b, c, d = state
        for i in range(64):
            if i < 16:
                f, g = (b & c) | (~b & d), i
            elif i < 32:
                f, g = (d & b) | (~d & c), (5 * i + 1) % 16
            elif i < 48:
                f, g = b ^ c ^ d, (3 * i + 5) % 16
            else:
                f, g = c ^ (b | ~d), (7 * i) % 16
            f = (f + a + _K[i] + m[g]) & 0xFFFFFFFF
            a, d, c = d, c, b
            b = (b + ((f << _S[i]) | (f >> (32 - _S[i])))) & 0xFFFFFFFF
        state = [(x + y) & 0xFFFFFFFF for x, y in zip(state, (a, b, c, d))]
    return b"".join(x.to_bytes(4, "little") for x in state)


# ---- the statement ---------------------------------------------------------------------------------------------------------------------
def statid_to_int(station_id: str, defect: str | None = None) -> int:
    assert defect is None or defect in DEFECTS, defect
    if defect == "no_strip_1c_1f":
        stripped = station_id.strip(" \t\n\r\x0b\x0c")
    elif defect == "strip_interior":
        stripped = "".join(station_id.split())
    else:
        stripped = station_id.strip()
    s = stripped.upper()
    if s and all(c in DIGITS for c in s):
        value = int(s, 36)
        return value % 2**64 if defect == "wrap_13_chars" and len(s) >= 13 else value
    if defect == "empty_is_zero" and not stripped:
        return 0
    message = (s if defect == "upper_before_md5" else stripped).encode()
    if defect in ("pad_single_block_only", "length_in_bytes_not_bits"):
        digest = md5_digest(message, single_block=defect == "pad_single_block_only", length_in_bytes=defect == "length_in_bytes_not_bits")
    else:
        digest = hashlib.md5(message).digest()
    return int.from_bytes(digest[:4], "big" if defect == "digest_big_endian" else "little", signed=False)


# ---- the kernel's view -----------------------------------------------------------------------------------------------------------------
def pack(strings: list[str], pitch_extra: int = 0, fill: int = 0) -> tuple[np.ndarray, int]:
    """``strings`` as a ``[n, width + pitch_extra]`` uint8 matrix of their UTF-8 bytes, zero-padded to ``width`` (the longest, at least
    1); the bytes beyond ``width`` hold ``fill``.  Returns the matrix and ``width``."""
    raw = [s.encode() for s in strings]
    width = max([len(b) for b in raw] + [1])
    out = np.full((len(raw), width + pitch_extra), fill, dtype=np.uint8)
    out[:, :width] = 0
    for i, b in enumerate(raw):
        out[i, :len(b)] = np.frombuffer(b, dtype=np.uint8)
    return out, width


def kernel_rules(text: np.ndarray, width: int) -> tuple[np.ndarray, list[bytes]]:
    """From the bytes alone: which rows the kernel leaves undecided, and every row's bytes up to ``end`` (what the host path sees of a
    decided row)."""
    text = np.asarray(text, dtype=np.uint8)[:, :width]
    n = text.shape[0]
    nonzero = text != 0
    end = np.where(nonzero.any(axis=1), width - np.argmax(nonzero[:, ::-1], axis=1), 0) if n else np.zeros(0, dtype=np.int64)
    undecided = (text >= 0x80).any(axis=1) | (nonzero.sum(axis=1) != end)
    rows = [text[i, :end[i]].tobytes() for i in range(n)]
    for i, row in enumerate(rows):
        if not undecided[i]:
            s = row.strip(ASCII_SPACE)
            if len(s) >= 13 and all(chr(c).upper() in DIGITS for c in s):
                undecided[i] = True
    return undecided, rows


def expected(text: np.ndarray, width: int) -> tuple[np.ndarray, np.ndarray]:
    """``(code int64 [n], undecided uint8 [n])`` of a launch over ``text``: the statement where the kernel decides, 0 where it does not."""
    undecided, rows = kernel_rules(text, width)
    code = np.zeros(len(rows), dtype=np.int64)
    for i, row in enumerate(rows):
        if not undecided[i]:
            code[i] = statid_to_int(row.decode("ascii"))
    return code, undecided.astype(np.uint8)


# ---- tables ----------------------------------------------------------------------------------------------------------------------------
def edge_strings() -> list[str]:
    """The edge table: every rule of the kernel at its boundary."""
    num = lambda n: ("Z9A0" * 64)[:n]  # noqa: E731  base-36 characters
    dash = lambda n: ("a-b_" * 64)[:n]  # noqa: E731  no number
    rows = ["here", "there", "1001"]  # the reference's three literals
    rows += ["", " ", "a-b", "-" * 56, "-" * 64, " ab ", "\x1c07\x1f", "1Y2P0IJ32E8E7", "1Y2P0IJ32E8E8"]
    for n in (1, 11, 12, 13, 55, 56, 63, 64, 65, 119, 120, 256):  # stripped lengths (0 is "" above)
        rows += [num(n), dash(n)]
    for b in (0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x1C, 0x1D, 0x1E, 0x1F, 0x20):
        rows += [chr(b) + "K7", "K7" + chr(b), "K" + chr(b) + "7"]
    rows += ["abc", "ABC", "aBc9", "zz", "ZZ", "0", "007", "a_b", "+1", "-1", "1.5", "0x1f", "\x08X", "\x0eX", "\x1bX", "\x21X", "\x7f"]
    rows += ["ı", "ſ", "ß", "\xa0x", "١", "xéy"]  # dotless i, long s, sharp s, no-break space, Arabic 1
    rows += ["a\x00b", "\x00ab"]  # a NUL before the last non-zero byte
    rows += ["  EGLL\t", "06 610", " 06610", "zzzzzzzzzzzz", "ZZZZZZZZZZZZZ", "0000000000001", " " * 13, "z" * 12 + " "]
    return rows


SEEDED_ROWS = (48, 300)


def seeded_strings(n: int) -> list[str]:
    """WMO-style numbers, ICAO-style letters, ids with ``-``, ``_`` and spaces, and edge rows (a few per cent undecided)."""
    rng = np.random.default_rng(20261020 + n)
    letters = "ABCDEFGHIJKLMNOPQRSTUVWXYZ"
    edges = [s for s in edge_strings() if len(s.encode()) <= 24 and statid_to_int(s) < 2**63]  # the seeded frames stay int64
    out = []
    for i in range(n):
        kind = rng.integers(0, 100)
        if kind < 45:
            s = f"{rng.integers(1000, 99999):05d}"
        elif kind < 65:
            s = "".join(letters[j] for j in rng.integers(0, 26, size=4))
            s = s.lower() if kind % 3 == 0 else s
        elif kind < 75:
            s = f" {rng.integers(1, 9999)} " if kind % 2 else f"{rng.integers(1, 999)}\t"
        elif kind < 90:
            sep = "-_ ."[int(rng.integers(0, 4))]
            s = "".join(letters[j] for j in rng.integers(0, 26, size=3)) + sep + str(rng.integers(0, 999))
        elif kind < 95:
            s = edges[int(rng.integers(0, len(edges)))]
        else:
            s = ["Zürich", "Ørland", "st\xa0x", "1Y2P0IJ32E8E6", "0BCDEFGHIJKLM"][int(rng.integers(0, 5))]
        out.append(s)
    return out


def golden() -> dict:
    with open(GOLDEN) as f:
        return json.load(f)


def strings_of(points: list[list[int]]) -> list[str]:
    return ["".join(chr(c) for c in row) for row in points]


def points_of(strings: list[str]) -> list[list[int]]:
    return [[ord(c) for c in s] for s in strings]
