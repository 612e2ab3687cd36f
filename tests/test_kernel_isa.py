"""CPU tier: the buffer descriptors of the reduction kernels stay in SGPRs.

A buffer load or store whose descriptor the compiler cannot prove
wave-uniform is wrapped in a waterfall loop (four v_readfirstlane, compares,
s_and_saveexec, the memory op, s_xor exec, s_cbranch_execnz): about twelve
instructions per memory op, and one loop finished before the next op issues.
reduce.hip makes a unit's descriptor inputs scalar once per unit (unit_body),
so no kernel should hold such a loop.  This test disassembles the gfx950 code
object inside the built library and checks, per kernel,

  * at most 8 v_readfirstlane, and
  * no s_and_saveexec / s_cbranch_execnz pair around a buffer_load or
    buffer_store,

for the default one-shot kernels of either engine (f32 and bf16, nt and
write-through stores), the default plan kernels and every k_program.  It
skips when the library is not built or the LLVM tools are not installed.
"""
import functools
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "hiccl_amd", "libhiccl_reduce.so")
LLVM = os.environ.get("HICCL_LLVM_BIN", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
MAX_READFIRSTLANE = 8

NS = "(anonymous namespace)::"
ONE_SHOT = [f"k_reduce_single<{NS}{op}, {shape}>" for op in ("OpF32", "OpBF16")
            for shape in ("256, 4, 11, 0", "256, 4, 31, 0", "512, 16, 11, 1", "512, 16, 31, 1")]
PLAN = [f"k_reduce_plan<{NS}{op}, {shape}>" for op in ("OpF32", "OpBF16")
        for shape in ("256, 4, 11, 0", "256, 4, 31, 0", "512, 16, 11, 1", "512, 16, 31, 1")]
PROGRAM = [f"k_program<{NS}{op}, {u}>" for op, us in (("OpF32", (2, 4)), ("OpBF16", (2, 4)), ("OpF64", (4,)),
                                                      ("OpU64", (4,)), ("OpI32", (4,)), ("OpRaw", (4,)))
           for u in us]


def tool(name):
    return os.path.join(LLVM, name)


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


@functools.lru_cache(maxsize=None)
def code_object():
    """Path of the library's gfx950 code object (taken out of its .hip_fatbin
    section), or a string saying why there is none."""
    if not os.path.exists(LIB):
        return None, f"{LIB} not built"
    for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-objdump"):
        if not os.path.exists(tool(t)):
            return None, f"{tool(t)} not installed"
    tmp = tempfile.mkdtemp(prefix="hiccl_isa_")
    fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "gfx950.co")
    try:
        run(tool("llvm-objcopy"), "--dump-section", f".hip_fatbin={fat}", LIB, os.path.join(tmp, "rest"))
        run(tool("clang-offload-bundler"), "--unbundle", "--type=o", f"--input={fat}", f"--targets={TARGET}",
            f"--output={co}")
    except subprocess.CalledProcessError as e:
        return None, f"no {TARGET} code object in {LIB}: {e.stderr.strip()[-300:]}"
    return co, ""


FUNC = re.compile(r"^([0-9a-f]+) .{7} \.text\t[0-9a-f]+ (?:\.protected )?(.+)$")


@functools.lru_cache(maxsize=None)
def kernel_symbols():
    """{demangled name: (mangled name, address)} of the code object's functions."""
    co, _ = code_object()
    funcs = lambda *flags: {m.group(1): m.group(2) for m in  # noqa: E731
                            map(FUNC.match, run(tool("llvm-objdump"), "-t", *flags, co).splitlines())
                            if m and " F " in m.group(0)}
    mangled, demangled = funcs(), funcs("-C")
    return {demangled[addr]: (name, int(addr, 16)) for addr, name in mangled.items()}


def find_symbol(name):
    """(mangled symbol, address) of the kernel whose demangled name holds `name`."""
    hits = [v for d, v in kernel_symbols().items() if name in d]
    assert len(hits) == 1, f"{name}: {len(hits)} kernels match"
    return hits[0]


INSTR = re.compile(r"^\s+([a-z][a-z0-9_]+)\b([^/]*)//\s*([0-9A-F]+):[^<]*(?:<[^>]*\+0x([0-9a-f]+)>)?")


def instructions(kernel):
    """(address, mnemonic, branch target or None) of every instruction of one kernel."""
    co, _ = code_object()
    symbol, base = find_symbol(kernel)
    ins = []
    for ln in run(tool("llvm-objdump"), "-d", f"--disassemble-symbols={symbol}", co).splitlines():
        m = INSTR.match(ln)
        if m:
            ins.append((int(m.group(3), 16), m.group(1), base + int(m.group(4), 16) if m.group(4) else None))
    assert len(ins) > 20 and ins[0][0] == base, f"{kernel}: disassembly not understood"
    return ins


def waterfalls(ins):
    """Addresses of the buffer loads and stores inside a one-block loop that
    an s_cbranch_execnz closes and that narrows exec with s_and_saveexec: the
    compiler's loop around a memory op whose descriptor it holds in VGPRs.
    (A unit loop that ends in s_cbranch_execnz has other branches inside.)"""
    bad = []
    for addr, op, target in ins:
        if op == "s_cbranch_execnz" and target is not None and target <= addr:
            body = [(a, o) for a, o, _ in ins if target <= a < addr]
            if any(o.startswith("s_and_saveexec") for _, o in body) and \
                    not any(o.startswith(("s_cbranch", "s_branch")) for _, o in body):
                bad += [a for a, o in body if o.startswith(("buffer_load", "buffer_store"))]
    return bad


@pytest.mark.parametrize("kernel", ONE_SHOT + PLAN + PROGRAM)
def test_descriptors_stay_scalar(kernel):
    co, why = code_object()
    if co is None:
        pytest.skip(why)
    ins = instructions(kernel)
    assert any(op.startswith("buffer_load_dwordx4") for _, op, _ in ins), f"{kernel}: no buffer loads found"
    rfl = sum(op.startswith("v_readfirstlane") for _, op, _ in ins)
    assert rfl <= MAX_READFIRSTLANE, f"{kernel}: {rfl} v_readfirstlane"
    bad = waterfalls(ins)
    assert not bad, f"{kernel}: {len(bad)} buffer ops inside a waterfall loop, first at {bad[0]:#x}"
