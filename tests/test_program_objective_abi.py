"""CPU checks of the objective-program boundary (include/bbopt_hip.h, bbo_program_create): the
library exports the two entry points, the structs a caller built against the earlier header uses
keep their size, and a program compiles -- or fails with the compiler's own words -- for an
architecture given by name, with no device on the machine."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ROSENBROCK = r"""
extern "C" __device__ double bbo_user_objective(const double *x, int n, const double *data)
{
    double s = 0.;
    for (int j = 0; j + 1 < n; j++) {
        const double t = x[j + 1] - x[j] * x[j], u = 1. - x[j];
        s += 100. * (t * t) + u * u;
    }
    return s;
}
"""

UNDECLARED = r"""
extern "C" __device__ double bbo_user_objective(const double *x, int n, const double *data)
{
    return x[0] + my_missing_scale;
}
"""

OTHER_NAME = r"""
extern "C" __device__ double some_other_objective(const double *x, int n, const double *data)
{
    return x[0];
}
"""

# names the function (in a comment and a declaration) but never defines it: only the linker notices
DECLARED_ONLY = r"""
extern "C" __device__ double bbo_user_objective(const double *x, int n, const double *data);
__device__ double helper(const double *x) { return x[0]; }
"""


def _create(source, arch=b"gfx950", data=None):
    from bboptpy_amd import _ffi
    L = _ffi.lib()
    h = C.c_void_p()
    if data is None:
        st = L.bbo_program_create(source.encode(), arch, None, 0, C.byref(h))
    else:
        arr = (C.c_double * len(data))(*data)
        st = L.bbo_program_create(source.encode(), arch, arr, len(data), C.byref(h))
    msg = L.bbo_last_error(None).decode(errors="replace")
    return st, h, msg


def test_library_exports_the_program_entry_points():
    from bboptpy_amd import _ffi
    lib = C.CDLL(_ffi.LIB_PATH)
    for name in ("bbo_program_create", "bbo_program_destroy"):
        assert hasattr(lib, name), "libbbopt_hip.so does not export %s" % name
        assert name in _ffi.EXPORTED_SYMBOLS
    assert _ffi.OBJ_PROGRAM == 3
    header = open(os.path.join(ROOT, "include", "bbopt_hip.h")).read()
    assert "BBO_OBJECTIVE_PROGRAM = 3" in header


def test_struct_sizes_are_unchanged():
    """bbo_objective and bbo_params as a caller built against the earlier header laid them out
    (x86-64: int, int, three pointers; the params end with stol and ranked)"""
    from bboptpy_amd import _ffi
    assert C.sizeof(_ffi.Objective) == 32
    assert _ffi.Objective.user.offset == 24
    assert C.sizeof(_ffi.Params) == _ffi.Params.pcauchy.offset + 8 + 16
    assert [f[0] for f in _ffi.Params._fields_][-2:] == ["stol", "ranked"]
    assert [f[0] for f in _ffi.Objective._fields_] == ["kind", "builtin", "scalar", "batch", "user"]


def test_valid_source_compiles_without_a_device():
    from bboptpy_amd import _ffi
    st, h, msg = _create(ROSENBROCK, data=[1., 2., 3.])
    assert st == 0, msg
    assert h.value
    assert _ffi.lib().bbo_program_destroy(h) == 0
    assert _ffi.lib().bbo_program_destroy(h) == -1       # no longer a live program
    st, h, msg = _create(ROSENBROCK)                      # data_count == 0
    assert st == 0, msg
    assert _ffi.lib().bbo_program_destroy(h) == 0


def test_undeclared_identifier_reports_the_compiler_log():
    st, h, msg = _create(UNDECLARED)
    assert st == -1 and not h.value
    assert "my_missing_scale" in msg
    # the user's own line and column: the identifier sits on line 4 of the source handed over
    assert "objective.hip:4:" in msg


@pytest.mark.parametrize("source", [OTHER_NAME, DECLARED_ONLY], ids=["other-name", "declared-only"])
def test_source_without_the_function_is_rejected(source):
    st, h, msg = _create(source)
    assert st == -1 and not h.value
    assert "bbo_user_objective" in msg and "does not define" in msg


def test_xnack_plus_is_refused():
    st, h, msg = _create(ROSENBROCK, arch=b"gfx950:xnack+")
    assert st == -1 and not h.value and "xnack+" in msg


def test_device_objective_raises_value_error_with_the_log():
    import bboptpy_amd as bb
    ok = bb.objectives.DeviceObjective(ROSENBROCK, arch="gfx950")
    assert bb.DeviceObjective is bb.objectives.DeviceObjective and ok._handle.value
    with pytest.raises(ValueError) as ei:
        bb.objectives.DeviceObjective(UNDECLARED, data=[1., 2.], arch="gfx950")
    assert "my_missing_scale" in str(ei.value) and "objective.hip:4:" in str(ei.value)
    with pytest.raises(ValueError) as ei:
        bb.objectives.DeviceObjective(OTHER_NAME, arch="gfx950")
    assert "bbo_user_objective" in str(ei.value)


def test_families_without_a_program_path_say_so():
    """(Python side; the library's own refusal at bbo_init needs a device: the GPU suite)"""
    import numpy as np
    import bboptpy_amd as bb
    prog = bb.DeviceObjective(ROSENBROCK, arch="gfx950")
    lo, up = -np.ones(4), np.ones(4)
    for alg in (bb.APSO(100, 1e-4, 8), bb.CSO(100, 1e-4, 9), bb.CCPSO(100, 1e-4, 8, [2, 4])):
        with pytest.raises(ValueError) as ei:
            alg.initialize(prog, lo, up, np.zeros(4))
        assert "CMAES" in str(ei.value) and "SHADE" in str(ei.value)


def test_library_works_without_hiprtc():
    """the run-time compiler is opened at the first bbo_program_create, not linked: with none to be
    found the library loads, everything else answers, and the call says what is missing"""
    code = (
        "import ctypes as C\n"
        "from bboptpy_amd import _ffi\n"
        "L = _ffi.lib()\n"
        "assert b'gfx950' in L.bbo_version()\n"
        "p = _ffi.default_params(_ffi.ALGO_ACTIVE_CMAES)\n"
        "assert p.populations == 1\n"
        "h = C.c_void_p()\n"
        "st = L.bbo_program_create(b'double bbo_user_objective;', b'gfx950', None, 0, C.byref(h))\n"
        "msg = L.bbo_last_error(None).decode()\n"
        "assert st == -1 and 'hiprtc' in msg and 'not available' in msg, (st, msg)\n"
        "print('OK')\n")
    env = dict(os.environ, BBO_HIPRTC_LIB="/nonexistent/libhiprtc-none.so",
               PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout + out.stderr
    if shutil.which("readelf") is None:
        return
    needed = subprocess.run(["readelf", "-d", os.path.join(ROOT, "bboptpy_amd", "libbbopt_hip.so")],
                            capture_output=True, text=True)
    if needed.returncode == 0:
        assert "NEEDED" in needed.stdout and "hiprtc" not in needed.stdout
