"""What every ctypes binding of this package shares: where its library is, loading it once with every prototype declared, and the
mapping of a C status to a Python exception.  No torch, no numpy: the ``native*`` modules build one ``Library`` each from their
``SIGNATURES``.
"""

from __future__ import annotations

import ctypes
import os
from typing import Any, Callable

LIB_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib")
OK, EINVAL = 0, -1  # ATX_OK, ATX_EINVAL (include/atx.h): the two statuses every library of the package returns


def plain_failure(fn: str, message: str, code: int) -> Exception:
    """A status that ``errors`` does not name, as the companion libraries report it: the message alone."""
    return RuntimeError(message)


class Library:
    """One shared library of ``lib/``: ``file_name`` there unless the variable ``env_var`` names another file, ``signatures`` as
    ``name -> (restype, argtypes)`` for every entry point of its header, ``last_error`` the entry point that returns the message of the
    calling thread's last failure.

    ``check`` turns a status into an exception: ``errors`` maps a status to the type raised with the message alone, ``unmapped`` makes
    the exception of every other status from ``(fn, message, code)``, and where the library left no message, ``strerror`` names the
    entry point that describes a status (without one the message is ``"<fn> failed with code <code>"``)."""

    def __init__(self, file_name: str, env_var: str, signatures: dict[str, tuple[Any, list[Any]]], last_error: str, *,
                 errors: dict[int, type[Exception]] | None = None, unmapped: Callable[[str, str, int], Exception] = plain_failure,
                 strerror: str | None = None) -> None:
        self.file_name, self.env_var, self.signatures, self.last_error = file_name, env_var, signatures, last_error
        self.errors = {EINVAL: ValueError} if errors is None else errors
        self.unmapped, self.strerror = unmapped, strerror
        self.handle: Any = None  # the library in use: None until load() or use()

    def path(self) -> str:
        """``lib/<file_name>`` next to this file; the environment variable overrides it."""
        return os.environ.get(self.env_var) or os.path.join(LIB_DIR, self.file_name)

    def open(self, path: str, older_build: bool = False) -> ctypes.CDLL:
        """A build of the library with every prototype declared; raises ``AttributeError`` if a symbol of the header is missing — unless
        ``older_build`` says the library may predate the header: its missing entry points are then left undeclared."""
        handle = ctypes.CDLL(path)
        for name, (restype, argtypes) in self.signatures.items():
            if older_build and not hasattr(handle, name):
                continue
            fn = getattr(handle, name)  # AttributeError if the symbol is not exported
            fn.restype, fn.argtypes = restype, argtypes
        return handle

    def load(self) -> Any:
        """The library in use; the first call opens ``path()``.  Raises if the file is absent or lacks a symbol of the header."""
        if self.handle is None:
            path = self.path()
            if not os.path.exists(path):
                raise RuntimeError(f"{path} not found: the HIP extension is not built. Run `python -c \"import __graft_entry__ as g; "
                                   "g.build()\"` (hipcc --offload-arch=gfx950) — this package has no CPU fallback.")
            self.handle = self.open(path)
        return self.handle

    def use(self, handle: Any) -> Any:
        """Route every call through ``handle`` (from ``open``) and return what was in use before; ``None`` goes back to ``load()``'s own."""
        before, self.handle = self.handle, handle
        return before

    def check(self, fn: str, code: int) -> None:
        """Raise what the status ``code`` of the entry point ``fn`` stands for; ``OK`` returns."""
        if code == OK:
            return
        handle = self.load()
        message = getattr(handle, self.last_error)().decode()
        if not message:
            message = getattr(handle, self.strerror)(code).decode() if self.strerror else f"{fn} failed with code {code}"
        if code in self.errors:
            raise self.errors[code](message)
        raise self.unmapped(fn, message, code)
