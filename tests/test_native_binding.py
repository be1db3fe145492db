"""``_binding.Library`` without a library: where it looks for its file, how it opens it, and which exception each of the five bindings
raises for which status.  The handle is a stub whose entry points return chosen codes, so nothing here needs a build or a GPU.

The table of exceptions is what the bindings raised when each had its own mapping: libatx and libatx_missing raise ``ValueError`` /
``AssertionError`` / ``NotImplementedError`` for ``EINVAL`` / ``ESHAPE`` / ``ENOTIMPL`` with the message alone and ``AtxError`` with the
entry point's name in front otherwise (libatx leaves the code out for ``ECOMM`` and describes a status without a message through
``atx_strerror``); libatx_text, libatx_plan and libatx_mesh raise ``ValueError`` for ``EINVAL`` and a plain ``RuntimeError`` otherwise.
"""

from __future__ import annotations

import ctypes
import os
import re
from ctypes import c_char_p, c_int, c_void_p

import pytest

from anemoi_transform_amd import _binding, native, native_mesh, native_missing, native_plan, native_text

EINVAL, ESHAPE, ENOTIMPL, EHIP, ECOMM, UNKNOWN = -1, -2, -3, -4, -7, -99
FN = "atx_some_entry_point"


def strerror_of(code: int) -> str:
    return f"status {code} described"


def libatx(code: int, said: str):
    message = said or strerror_of(code)
    return {EINVAL: (ValueError, message), ESHAPE: (AssertionError, message), ENOTIMPL: (NotImplementedError, message),
            ECOMM: (native.AtxError, f"{FN}: {message}")}.get(code, (native.AtxError, f"{FN}: {message} (code {code})"))


def libatx_missing(code: int, said: str):
    message = said or f"{FN} failed with code {code}"
    return {EINVAL: (ValueError, message), ESHAPE: (AssertionError, message), ENOTIMPL: (NotImplementedError, message)}.get(
        code, (native.AtxError, f"{FN}: {message} (code {code})"))


def companion(code: int, said: str):
    message = said or f"{FN} failed with code {code}"
    return (ValueError if code == EINVAL else RuntimeError), message


# binding module, its last-error entry point, what it raises for (status, message of the library)
BINDINGS = [(native, "atx_last_error", libatx), (native_missing, "atx_missing_last_error", libatx_missing),
            (native_text, "atx_text_last_error", companion), (native_plan, "atx_plan_last_error", companion),
            (native_mesh, "atx_mesh_last_error", companion)]


class Stub:
    """A handle whose one entry point returns ``code`` and whose last-error entry point returns ``said``."""

    def __init__(self, last_error: str, code: int, said: str) -> None:
        setattr(self, last_error, lambda: said.encode())
        setattr(self, FN, lambda *args: code)
        self.atx_strerror = lambda status: strerror_of(status).encode()


@pytest.fixture
def stubbed():
    """``stubbed(module, stub)`` routes the module's library through the stub until the test ends."""
    undo = []

    def install(module, stub):
        undo.append((module.LIBRARY, module.LIBRARY.use(stub)))

    yield install
    for library, before in reversed(undo):
        library.use(before)


@pytest.mark.parametrize("said", ["", "n_tgt = -3 is negative"], ids=["no-message", "message"])
@pytest.mark.parametrize("code", [EINVAL, ESHAPE, ENOTIMPL, EHIP, ECOMM, UNKNOWN], ids=["EINVAL", "ESHAPE", "ENOTIMPL", "EHIP", "ECOMM", "unknown"])
@pytest.mark.parametrize("module, last_error, expected", BINDINGS, ids=[b[0].__name__.rsplit(".", 1)[-1] for b in BINDINGS])
def test_status_to_exception(stubbed, module, last_error, expected, code, said):
    stubbed(module, Stub(last_error, code, said))
    kind, message = expected(code, said)
    with pytest.raises(Exception) as raised:
        module.LIBRARY.check(FN, code)
    assert type(raised.value) is kind and str(raised.value) == message
    if hasattr(module, "_call"):  # libatx and libatx_missing call every entry point through one function
        with pytest.raises(Exception) as raised:
            module._call(FN, 1, 2)
        assert type(raised.value) is kind and str(raised.value) == message


@pytest.mark.parametrize("module, last_error, expected", BINDINGS, ids=[b[0].__name__.rsplit(".", 1)[-1] for b in BINDINGS])
def test_ok_raises_nothing(stubbed, module, last_error, expected):
    stubbed(module, Stub(last_error, 0, "left over from an earlier call"))
    assert module.LIBRARY.check(FN, 0) is None and module.OK == 0 and module.EINVAL == EINVAL
    if hasattr(module, "_call"):
        assert module._call(FN) is None


def test_status_constants_and_module_names():
    assert (native.OK, native.EINVAL, native.ESHAPE, native.ENOTIMPL, native.EHIP, native.ECOMM) == (0, EINVAL, ESHAPE, ENOTIMPL, EHIP, ECOMM)
    assert (native_missing.EINVAL, native_missing.ESHAPE, native_missing.ENOTIMPL) == (EINVAL, ESHAPE, ENOTIMPL)
    assert issubclass(native.AtxError, RuntimeError)
    for module, _, _ in BINDINGS:
        assert module.lib_path == module.LIBRARY.path and module.load == module.LIBRARY.load and module.LIBRARY.signatures is module.SIGNATURES
    assert native.open_library == native.LIBRARY.open and native.use_library == native.LIBRARY.use
    for module in (native_text, native_plan, native_mesh, _binding):  # these stand without libatx's binding
        assert not re.search(r"^from \.native import|^from \. import .*\bnative\b", open(module.__file__).read(), flags=re.M)
    assert not re.search(r"^\s*(import|from) (torch|numpy)\b", open(_binding.__file__).read(), flags=re.M)


@pytest.mark.parametrize("module, variable, file_name", [
    (native, "ATX_LIBRARY", "libatx.so"), (native_text, "ATX_TEXT_LIBRARY", "libatx_text.so"), (native_plan, "ATX_PLAN_LIBRARY", "libatx_plan.so"),
    (native_mesh, "ATX_MESH_LIBRARY", "libatx_mesh.so"), (native_missing, "ATX_MISSING_LIBRARY", "libatx_missing.so")],
    ids=["native", "native_text", "native_plan", "native_mesh", "native_missing"])
def test_the_environment_names_another_file(monkeypatch, module, variable, file_name):
    monkeypatch.delenv(variable, raising=False)
    assert module.lib_path() == os.path.join(os.path.dirname(os.path.abspath(module.__file__)), "lib", file_name)
    monkeypatch.setenv(variable, "/elsewhere/libother.so")
    assert module.lib_path() == "/elsewhere/libother.so"


def test_a_missing_file_is_not_built(monkeypatch, tmp_path):
    library = _binding.Library("libatx_nothing.so", "ATX_NOTHING_LIBRARY", {}, "atx_nothing_last_error")
    absent = str(tmp_path / "libatx_nothing.so")
    monkeypatch.setenv("ATX_NOTHING_LIBRARY", absent)
    with pytest.raises(RuntimeError) as raised:
        library.load()
    assert str(raised.value) == (f"{absent} not found: the HIP extension is not built. Run `python -c \"import __graft_entry__ as g; "
                                 "g.build()\"` (hipcc --offload-arch=gfx950) — this package has no CPU fallback.")
    assert type(raised.value) is RuntimeError and library.handle is None


def some_library() -> str:
    """A shared object that is on every machine: the extension module under ctypes itself.  It exports its init function."""
    import _ctypes

    return getattr(_ctypes, "__file__", None) or pytest.skip("_ctypes is built into this interpreter")


def test_open_declares_prototypes_and_misses_a_symbol_only_for_an_older_build():
    signatures = {"PyInit__ctypes": (c_void_p, []), "atx_entry_point_of_a_later_header": (c_int, [c_char_p])}
    library = _binding.Library("libatx_nothing.so", "ATX_NOTHING_LIBRARY", signatures, "atx_nothing_last_error")
    with pytest.raises(AttributeError):
        library.open(some_library())
    handle = library.open(some_library(), older_build=True)
    assert handle.PyInit__ctypes.restype is c_void_p and handle.PyInit__ctypes.argtypes == []
    assert library.handle is None  # open() does not put the build to use
    complete = _binding.Library("libatx_nothing.so", "ATX_NOTHING_LIBRARY", {"PyInit__ctypes": (c_void_p, [])}, "atx_nothing_last_error")
    assert complete.open(some_library()).PyInit__ctypes.restype is c_void_p


def test_use_swaps_the_handle_and_none_goes_back_to_load(monkeypatch):
    library = _binding.Library("libatx_nothing.so", "ATX_NOTHING_LIBRARY", {"PyInit__ctypes": (c_void_p, [])}, "atx_nothing_last_error")
    monkeypatch.setenv("ATX_NOTHING_LIBRARY", some_library())
    first, second = object(), object()
    assert library.use(first) is None and library.load() is first
    assert library.use(second) is first and library.load() is second
    assert library.use(None) is second and library.handle is None
    own = library.load()
    assert isinstance(own, ctypes.CDLL) and own.PyInit__ctypes.restype is c_void_p and library.load() is own  # opened once
    assert library.use(first) is own
