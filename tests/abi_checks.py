"""What the host tests of the five libraries share: a library's dynamic symbol table, read with ``nm``, and the declarations that its
header marks with its export macro."""

from __future__ import annotations

import os
import re
import shutil
import subprocess

import pytest


def nm_tool() -> str | None:
    """``nm``, or ROCm's ``llvm-nm``; ``None`` where there is neither."""
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    return nm if shutil.which("nm") or os.path.exists(nm) else None


def defined_dynamic_symbols(lib_path: str) -> tuple[list[str], set[str]]:
    """``(names, kinds)`` of the symbols that the library defines in its dynamic table: the names sorted and without their version
    suffix, the kinds as nm's letters (``T``: a function in the text section, not weak).  Skips the calling test where there is no nm."""
    nm = nm_tool() or pytest.skip("no nm")
    listing = subprocess.run([nm, "-D", "--defined-only", lib_path], capture_output=True, text=True, check=True).stdout
    lines = [line for line in listing.splitlines() if line.strip()]
    return sorted(line.split()[-1].split("@")[0] for line in lines), {line.split()[-2] for line in lines}


def header_declarations(header: str, macro: str) -> list[str]:
    """The entry points that ``header`` declares with ``macro`` outside its comments, in header order."""
    text = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    return re.findall(r"^%s [^;(]*?\b(atx_[a-z_0-9]+)\s*\(" % macro, text, flags=re.M)
