"""CPU checks of JAYA at the drop-in boundary: the Python signature against
tests/golden/class_surface.json, bbo_jaya_params_default, the untouched layout of bbo_params, and
the statuses of bbo_jaya_configure that need no handle (the ones that need a device-backed handle
are in tests/test_jaya_gpu.py: without a GPU bbo_create returns BBO_ERR_NO_DEVICE)."""
import ctypes as C
import inspect
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _surface():
    with open(os.path.join(ROOT, "tests", "golden", "class_surface.json")) as fh:
        return json.load(fh)["classes"]["JAYA"]


def test_class_surface_matches_the_reference():
    import bboptpy_amd as bb
    ref = _surface()
    E = inspect.Parameter.empty
    cls = bb.JAYA
    ps = inspect.signature(cls.__init__).parameters
    mine = [(k, v.default) for k, v in ps.items() if k not in ("self", "ext")]
    want = [(kw["name"], E if kw["required"] else kw["default"]) for kw in ref["init"]["keywords"]]
    assert [k for k, _ in mine] == [k for k, _ in want]
    assert [k for k, _ in mine] == ["mfev", "tol", "np", "npmin", "adapt", "k0", "mutation", "scale",
                                    "beta", "kcheb", "temper"]
    for (k, got), (_, exp) in zip(mine, want):
        assert (got is E) == (exp is E), k
        if exp is E:
            continue
        if isinstance(exp, dict):       # an enumerator: {"cxx": "JayaSearch::jaya_mutation_method::logistic"}
            assert isinstance(got, cls.JAYA_Mutation) and got.name == exp["cxx"].split("::")[-1], k
        else:
            assert got == exp and type(got) is type(exp), (k, got, exp)
    assert any(v.kind is inspect.Parameter.VAR_KEYWORD for v in ps.values())
    assert ref["base"] == "MultivariateSearch" and bb.MultivariateSearch in cls.__mro__[1:]
    assert "JAYA" in bb.__all__ and cls._accepts_program is False
    for name in ("optimize", "initialize", "iterate", "solution"):
        assert callable(getattr(cls, name))


def test_mutation_enum_is_nested_and_exported():
    import enum
    import bboptpy_amd as bb
    M = bb.JAYA.JAYA_Mutation
    assert issubclass(M, enum.IntEnum)
    assert [(m.name, int(m)) for m in M] == [("original", 0), ("levy", 1), ("tent_map", 2), ("logistic", 3)]
    for m in M:                          # pybind's export_values
        assert getattr(bb.JAYA, m.name) is m


def test_constructor_marshals_both_structs():
    import bboptpy_amd as bb
    from bboptpy_amd import _ffi
    assert bb.JAYA._algo == _ffi.ALGO_JAYA == 12
    a = bb.JAYA(5000, 1e-6, 40, 5, seed=9, populations=3)
    p, j = a._params, a._jaya
    assert (p.algo, p.mfev, p.tol, p.np, p.npmin, p.seed, p.populations) == (12, 5000, 1e-6, 40, 5, 9, 3)
    assert (j.adapt, j.k0, j.mutation, j.kcheb, j.scale, j.beta, j.temper) == (1, 2, 3, 2, 0.01, 1.5, 10.)
    b = bb.JAYA(5000, 1e-6, 40, 5, False, 4, bb.JAYA.levy, 0.02, 1.2, 3, 5.)
    j = b._jaya
    assert (j.adapt, j.k0, j.mutation, j.kcheb, j.scale, j.beta, j.temper) == (0, 4, 1, 3, 0.02, 1.2, 5.)
    assert bb.JAYA(1, 0., 4, 2, mutation=2)._jaya.mutation == 2
    with pytest.raises(ValueError):
        bb.JAYA(1, 0., 4, 2, mutation=4)


def test_jaya_params_default_and_untouched_bbo_params():
    from bboptpy_amd import _ffi
    L = _ffi.lib()
    j = _ffi.JayaParams()
    C.memset(C.byref(j), 0xA5, C.sizeof(j))
    L.bbo_jaya_params_default(C.byref(j))
    assert (j.adapt, j.k0, j.mutation, j.kcheb, j.scale, j.beta, j.temper) == (1, 2, 3, 2, 0.01, 1.5, 10.)
    assert C.sizeof(_ffi.JayaParams) == 4 * 4 + 3 * 8
    L.bbo_jaya_params_default(None)     # tolerated
    # bbo_params keeps its size and its last fields; JAYA writes nothing past the base struct
    base = _ffi.Params.stol.offset
    assert base == _ffi.Params.pcauchy.offset + 8 and C.sizeof(_ffi.Params) == base + 16
    fn = C.CDLL(_ffi.LIB_PATH).bbo_params_default
    fn.argtypes, fn.restype = [C.c_void_p, C.c_int], None
    buf = (C.c_ubyte * (base + 64))(*([0xA5] * (base + 64)))
    fn(C.addressof(buf), _ffi.ALGO_JAYA)
    assert bytes(buf[base:]) == b"\xA5" * 64 and C.c_int.from_buffer(buf, 0).value == 12


def test_configure_without_a_handle_is_an_argument_error():
    from bboptpy_amd import _ffi
    L = _ffi.lib()
    j = _ffi.JayaParams()
    L.bbo_jaya_params_default(C.byref(j))
    assert L.bbo_jaya_configure(None, C.byref(j)) == _ffi.ERR_ARG
    for name in ("bbo_jaya_params_default", "bbo_jaya_configure"):
        assert name in _ffi.EXPORTED_SYMBOLS
