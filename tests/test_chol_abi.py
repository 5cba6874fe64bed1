"""CPU checks of CholeskyCMAES at the drop-in boundary: bbo_params_default and the Python
signature against tests/golden/class_surface.json (the logic of tests/test_abi.py)."""
import inspect
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _surface():
    with open(os.path.join(ROOT, "tests", "golden", "class_surface.json")) as fh:
        return json.load(fh)["classes"]["CholeskyCMAES"]


def test_default_parameters_are_the_reference_defaults():
    import bboptpy_amd as bb
    from bboptpy_amd import _ffi
    assert bb.CholeskyCMAES._algo == _ffi.ALGO_CHOLESKY_CMAES == 11
    p = _ffi.default_params(_ffi.ALGO_CHOLESKY_CMAES)
    assert p.algo == 11
    checked = 0
    for kw in _surface()["init"]["keywords"]:
        if kw["required"]:
            continue
        want = kw["default"]
        assert getattr(p, kw["name"]) == (int(want) if isinstance(want, bool) else want), kw["name"]
        checked += 1
    assert checked == 2
    assert p.ranked == 0 and p.stol == 0. and p.populations == 1      # the extension is off
    # appended fields: everything the struct held before keeps its place
    names = [f[0] for f in _ffi.Params._fields_]
    assert names[-2:] == ["stol", "ranked"] and names[-3] == "pcauchy"


def test_class_surface_matches_the_reference():
    import bboptpy_amd as bb
    ref = _surface()
    E = inspect.Parameter.empty
    cls = bb.CholeskyCMAES
    ps = inspect.signature(cls.__init__).parameters
    mine = [(k, v.default) for k, v in ps.items() if k not in ("self", "ext")]
    want = [(kw["name"], E if kw["required"] else kw["default"]) for kw in ref["init"]["keywords"]]
    assert [k for k, _ in mine] == [k for k, _ in want]
    for (k, got), (_, exp) in zip(mine, want):
        assert (got is E) == (exp is E), k
        if exp is not E:
            assert got == exp and type(got) is type(exp), (k, got, exp)
    assert any(v.kind is inspect.Parameter.VAR_KEYWORD for v in ps.values())
    assert ref["base"] == "BaseCMAES" and getattr(bb, ref["base"]) in cls.__mro__[1:]
    assert "CholeskyCMAES" in bb.__all__
    for name in ("optimize", "initialize", "iterate", "solution"):
        assert callable(getattr(cls, name))


def test_constructor_carries_the_extensions():
    import bboptpy_amd as bb
    a = bb.CholeskyCMAES(1000, 1e-6, 1e-7, 12, seed=5, populations=3, poll_every=2, ranked=True)
    p = a._params
    assert (p.mfev, p.tol, p.stol, p.np, p.sigma0, p.bound) == (1000, 1e-6, 1e-7, 12, 2., 0)
    assert (p.seed, p.populations, p.poll_every, p.ranked) == (5, 3, 2, 1)
    assert bb.CholeskyCMAES(1000, 1e-6, 1e-7, 12, 3., True)._params.bound == 1
    # a legal base of the restart drivers
    bb.IPopCMAES(bb.CholeskyCMAES(1000, 1e-6, 1e-7, 12), 5000)
    bb.BiPopCMAES(bb.CholeskyCMAES(1000, 1e-6, 1e-7, 12), 5000)


def test_callers_built_against_the_shorter_struct_stay_binary_compatible():
    """a program compiled before `stol` / `ranked` existed holds a struct that ends where `stol`
    begins: for its algorithms bbo_params_default must not write past that end"""
    import ctypes as C
    from bboptpy_amd import _ffi
    base = _ffi.Params.stol.offset
    assert base == _ffi.Params.pcauchy.offset + 8 and C.sizeof(_ffi.Params) == base + 16
    fn = C.CDLL(_ffi.LIB_PATH).bbo_params_default
    fn.argtypes, fn.restype = [C.c_void_p, C.c_int], None
    for algo in range(11):
        buf = (C.c_ubyte * (base + 64))(*([0xA5] * (base + 64)))
        fn(C.addressof(buf), algo)
        assert bytes(buf[base:]) == b"\xA5" * 64, algo
        assert C.c_int.from_buffer(buf, 0).value == algo
    buf = (C.c_ubyte * (base + 64))(*([0xA5] * (base + 64)))
    fn(C.addressof(buf), _ffi.ALGO_CHOLESKY_CMAES)
    assert bytes(buf[base:base + 16]) == b"\x00" * 16 and bytes(buf[base + 16:]) == b"\xA5" * 48
