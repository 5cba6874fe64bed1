"""CPU: the prefetch ring of cma_gram128s stays in flight, read off the SHIPPED library.

Every wavefront of the kernel streams its X fragments four k-steps ahead through a register ring
(bbo_cma_kernels.hpp, gram128_stream).  The vector-memory counter retires in order, so one
instruction in the chunk loop that uses the YOUNGEST load at once -- `s_waitcnt vmcnt(0)` -- drains
the whole ring and adds a memory round trip per chunk (round 10: a select on the rank just loaded did
exactly that).  This test disassembles bboptpy_amd/libbbopt_hip.so (llvm-objdump from /opt/rocm, no
GPU needed) and checks that

  1. the kernel has exactly four loop bodies that hold fp64 MFMAs -- one per wavefront role, the
     table and the look-up form of the coefficients sharing it (a loop body: an instruction range
     closed by a backward branch);
  2. none of them holds an `s_waitcnt` whose vmcnt field is 0;
  3. nor one that leaves fewer loads out than the three ring slots behind the one being swept hold
     (round 10 met vmcnt(3) twice on the way: a register shared with a load just issued).
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "bboptpy_amd", "libbbopt_hip.so")
LLVM = "/opt/rocm/lib/llvm/bin"
KERNEL = "cma_gram128s"
MFMA = "v_mfma_f64_16x16x4_f64"
RING_IN_FLIGHT = 3 * 5        # three slots behind the one a k-step sweeps, 5 or 6 fragment loads each


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    """[(address, instruction text)] of the kernel"""
    objdump = os.path.join(LLVM, "llvm-objdump")
    if not os.path.exists(objdump):
        pytest.skip("no llvm-objdump under /opt/rocm")
    assert os.path.exists(LIB), "libbbopt_hip.so is not built"
    d = tmp_path_factory.mktemp("isa")
    so = os.path.join(d, "lib.so")
    shutil.copy(LIB, so)            # (--offloading writes the bundles NEXT to its input)
    subprocess.run([objdump, "--offloading", so], check=True, capture_output=True)
    objs = [os.path.join(d, f) for f in sorted(os.listdir(d)) if "gfx950" in f]
    assert objs, "no gfx950 code objects in the library"
    for o in objs:
        syms = subprocess.run([objdump, "-t", o], check=True, capture_output=True, text=True).stdout
        m = re.search(r"\s(_ZN3bbo%d%sE\w*)\n" % (len(KERNEL), KERNEL), syms)
        if not m:
            continue
        out = subprocess.run([objdump, "-d", "--disassemble-symbols=" + m.group(1), o], check=True,
                             capture_output=True, text=True).stdout
        ins = []
        for line in out.splitlines():
            # "\ts_waitcnt vmcnt(0)      // 000000001234: BF8C0F70"
            m2 = re.match(r"^\s+(\S.*?)\s*//\s*([0-9A-Fa-f]+):", line)
            if m2:
                ins.append((int(m2.group(2), 16), m2.group(1).strip()))
        return ins
    raise AssertionError("kernel %s not found in the library" % KERNEL)


def _mfma_loops(ins):
    """(first, last) instruction indices of the loop bodies that hold an MFMA.  Backward branches to
    one header close one loop (the table and the look-up tail each jump back on their own): its body
    runs to the last of them.  A range that wraps another loop's is no body of its own -- the
    compiler lays the four wavefront roles out with long backward jumps between them -- and is dropped."""
    addr_to_idx = {a: k for k, (a, _) in enumerate(ins)}
    ends = {}
    for k, (a, t) in enumerate(ins):
        m = re.match(r"s_c?branch\w*\s+(-?\d+)", t)
        if not m:
            continue
        off = int(m.group(1))
        if off >= 32768:
            off -= 65536
        if off >= 0:
            continue
        target = a + 4 + 4 * off
        assert target in addr_to_idx, "backward branch to an address outside the listing: %s" % t
        first = addr_to_idx[target]
        if any(MFMA in ins[j][1] for j in range(first, k + 1)):
            ends[first] = max(ends.get(first, 0), k)
    ranges = sorted(ends.items())
    return [(a, b) for a, b in ranges
            if not any((c, e) != (a, b) and a <= c and e <= b for c, e in ranges)]


def _vmcnt(t):
    """the vmcnt field of an s_waitcnt, None where it does not wait on it"""
    m = re.search(r"vmcnt\((\d+)\)", t)
    if m:
        return int(m.group(1))
    m = re.match(r"s_waitcnt\s+(0x[0-9a-fA-F]+|\d+)$", t)      # (a raw immediate: gfx9 keeps vmcnt in bits 3:0 and 15:14)
    if m:
        imm = int(m.group(1), 0)
        return (imm & 0xf) | ((imm >> 14) & 0x3) << 4
    return None


def test_four_mfma_loops_and_no_drain_in_any(listing):
    ins = listing
    assert len(ins) > 1000, len(ins)
    loops = _mfma_loops(ins)
    assert len(loops) == 4, "loop bodies with fp64 MFMAs: %s" % [(ins[a][0], ins[b][0]) for a, b in loops]
    for first, last in loops:
        body = [t for _, t in ins[first:last + 1]]
        assert sum(MFMA in t for t in body) == 72, "8 k-steps of 9 tiles expected in a chunk"
        waits = [(t, _vmcnt(t)) for t in body if t.startswith("s_waitcnt") and _vmcnt(t) is not None]
        assert waits, "no vector-memory wait at all in a chunk loop?"
        drains = [t for t, v in waits if v == 0]
        assert not drains, "the chunk loop at %#x drains the ring: %s" % (ins[first][0], drains)
        # (stricter than `not 0`: a k-step's wait leaves the three younger slots in flight, at least
        # five fragments each; a wait that leaves fewer than 15 loads out has cut into the ring)
        cuts = [t for t, v in waits if v < RING_IN_FLIGHT]
        assert not cuts, "the chunk loop at %#x waits into the ring: %s" % (ins[first][0], cuts)
