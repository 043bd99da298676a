"""CPU-side checks of the product library: it builds for gfx950, loads, and
exports every symbol include/arroyo_amd.h declares.  No compute calls (no
GPU here); creation failure without a device must be loud."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "arroyo_amd", "libarroyo_amd.so")

def declared_symbols():
    """Every arroyo_amd_* function include/arroyo_amd.h declares."""
    import re
    hdr = open(os.path.join(ROOT, "include", "arroyo_amd.h")).read()
    syms = sorted(set(re.findall(r"\b(arroyo_amd_[a-z0-9_]+)\s*\(", hdr)))
    assert len(syms) > 40, syms  # all seven families + shared helpers
    return syms


SYMBOLS = declared_symbols()


def _build():
    from arroyo_amd import gpu
    return gpu.build()


def test_library_builds_and_exports_all_symbols():
    so = _build()
    lib = ctypes.CDLL(so)
    for sym in SYMBOLS:
        assert getattr(lib, sym, None) is not None, f"missing symbol {sym}"


def test_device_code_is_gfx950():
    import subprocess
    so = _build()
    out = subprocess.run(
        ["/opt/rocm/lib/llvm/bin/llvm-objdump", "--offloading", so],
        capture_output=True, text=True)
    assert "gfx950" in out.stdout + out.stderr


def test_create_without_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present; covered by -m gpu tests")
    from arroyo_amd import cabi, gpu
    lib = gpu.lib()
    cfg = cabi.make_config(width_ns=10**9, slide_ns=10**9,
                           aggs=[(cabi.COUNT, -1)])
    fn = cabi.bind(lib, "arroyo_amd_")
    h = fn["create"](ctypes.byref(cfg))
    assert not h, "create must fail without a HIP device (no CPU fallback)"
    msg = fn["last_error"](None).decode()
    assert "hip" in msg.lower() or "device" in msg.lower()


# ---- the ctypes mirrors against the headers they mirror --------------------

def _mirrors():
    from arroyo_amd import cabi
    return {t.__name__: t for t in vars(cabi).values()
            if isinstance(t, type) and issubclass(t, ctypes.Structure)
            and t is not ctypes.Structure}


def _header_constants(hdr):
    import re
    # comments speak of groups as "AMD_JOIN_*": a name ends in [A-Z0-9]
    return sorted(set(re.findall(
        r"\b(AMD_(?:AGG_|MOP_|JOIN_|SHUF_|MAX_AGGS|MAP_MAX_)"
        r"(?:[A-Z0-9_]*[A-Z0-9])?)\b(?!\*)", hdr)))


@pytest.fixture(scope="module")
def header_facts(tmp_path_factory):
    """What the host C compiler makes of include/arroyo_amd_types.h: a C
    program generated from the ctypes mirrors prints sizeof / offsetof for
    every mirrored struct and field, and the value of every AMD_* constant."""
    import subprocess
    inc = os.path.join(ROOT, "include")
    hdr = open(os.path.join(inc, "arroyo_amd_types.h")).read()
    lines = ["#include <stdio.h>", "#include <stddef.h>",
             '#include "arroyo_amd_types.h"', "int main(void) {"]
    for name, t in sorted(_mirrors().items()):
        lines.append(f'printf("S {name} %zu\\n", sizeof({name}));')
        for field in t._fields_:
            lines.append(f'printf("F {name}.{field[0]} %zu\\n", '
                         f'offsetof({name}, {field[0]}));')
    for const in _header_constants(hdr):
        lines.append(f'printf("C {const} %lld\\n", (long long)({const}));')
    lines += ["return 0;", "}"]
    d = tmp_path_factory.mktemp("layout")
    src, exe = d / "layout.c", d / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(["gcc", "-std=c11", "-I", inc, "-o", str(exe), str(src)],
                   check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True,
                         text=True).stdout
    facts = {"S": {}, "F": {}, "C": {}}
    for line in out.splitlines():
        kind, name, value = line.split()
        facts[kind][name] = int(value)
    return hdr, facts


def test_struct_mirrors_match_header_layout(header_facts):
    import re
    hdr, facts = header_facts
    mirrors = _mirrors()
    typedefs = re.findall(r"typedef\s+struct\s*\{.*?\}\s*(Amd\w+)\s*;", hdr,
                          re.S)
    assert len(typedefs) >= 13, typedefs
    assert set(typedefs) == set(mirrors), \
        "every typedef struct of the header has exactly one ctypes mirror"
    entries, bad = 0, []
    for name, t in mirrors.items():
        entries += 1
        if facts["S"][name] != ctypes.sizeof(t):
            bad.append((name, facts["S"][name], ctypes.sizeof(t)))
        for field in t._fields_:
            entries += 1
            c_off = facts["F"][f"{name}.{field[0]}"]
            if c_off != getattr(t, field[0]).offset:
                bad.append((f"{name}.{field[0]}", c_off,
                            getattr(t, field[0]).offset))
    print(f"{len(mirrors)} structs, {entries} entries, {len(bad)} mismatches")
    assert entries == len(facts["S"]) + len(facts["F"])
    assert not bad, f"(what, C, ctypes): {bad}"


def test_constants_match_header(header_facts):
    from arroyo_amd import cabi
    _, facts = header_facts
    consts = facts["C"]
    twins = {}
    for name in consts:
        for c_prefix, py_prefix in (("AMD_AGG_", ""), ("AMD_MOP_", "MOP_"),
                                    ("AMD_JOIN_", "JOIN_"),
                                    ("AMD_SHUF_", "AMD_SHUF_")):
            if name.startswith(c_prefix):
                twins[name] = getattr(cabi, py_prefix + name[len(c_prefix):],
                                      None)
    # every enum / define of these four groups has a Python twin today
    assert len(twins) == 28 + 21 + 4 + 7, sorted(twins)
    assert None not in twins.values(), \
        [n for n, v in twins.items() if v is None]
    # array lengths the mirrors spell as literals
    length = lambda t, f: dict((x[0], x[1]) for x in t._fields_)[f]._length_
    for t, f in ((cabi.AmdWindowConfig, "agg_ops"),
                 (cabi.AmdWindowConfig, "agg_col"),
                 (cabi.AmdSessionConfig, "agg_ops"),
                 (cabi.AmdSessionConfig, "agg_col"),
                 (cabi.AmdUpdatingConfig, "agg_ops"),
                 (cabi.AmdUpdatingConfig, "agg_col"),
                 (cabi.AmdUpdatingConfig, "agg_col2")):
        assert length(t, f) == consts["AMD_MAX_AGGS"], (t, f)
    assert length(cabi.AmdMapConfig, "prog") == consts["AMD_MAP_MAX_PROG"]
    assert length(cabi.AmdMapConfig, "out_reg") == consts["AMD_MAP_MAX_OUT"]
    assert length(cabi.AmdMapConfig, "out_is_f64") == \
        consts["AMD_MAP_MAX_OUT"]
    assert length(cabi.AmdShuffleOut, "cols") == consts["AMD_SHUF_MAX_COLS"]
    assert length(cabi.AmdShuffleOut, "row_start") == \
        consts["AMD_SHUF_MAX_PARTS"] + 1
    assert length(cabi.AmdShuffleOut, "byte_start") == \
        consts["AMD_SHUF_MAX_PARTS"] + 1
    assert len(cabi.SHUF_KERNEL_NAMES) == consts["AMD_SHUF_N_KERNELS"]
    for name, want in consts.items():
        if name in twins:
            assert twins[name] == want, (name, twins[name], want)


# ---- the prototype table ---------------------------------------------------

def test_prototype_table_covers_header():
    import re

    from arroyo_amd import cabi
    assert {"arroyo_amd_" + n for n in cabi.PROTOTYPES} == set(SYMBOLS)
    hdr = open(os.path.join(ROOT, "include", "arroyo_amd.h")).read()
    # the file's leading comment mentions functions in prose; declarations
    # start after the include guard
    decls = re.findall(r"\b(arroyo_amd_[a-z0-9_]+)\s*\(([^)]*)\)\s*;",
                       hdr[hdr.index("#ifndef ARROYO_AMD_H"):])
    assert sorted(n for n, _ in decls) == SYMBOLS
    for sym, params in decls:
        params = params.strip()
        n_params = 0 if params in ("", "void") else len(params.split(","))
        _, argtypes = cabi.PROTOTYPES[sym[len("arroyo_amd_"):]]
        assert len(argtypes) == n_params, sym


def _assert_declared(lib, prefix, require_all):
    from arroyo_amd import cabi
    seen = 0
    for name, (restype, argtypes) in cabi.PROTOTYPES.items():
        f = getattr(lib, prefix + name, None)
        if f is None:
            assert not require_all, f"missing symbol {prefix}{name}"
            continue
        seen += 1
        assert f.argtypes is not None, prefix + name
        assert list(f.argtypes) == list(argtypes), prefix + name
        assert f.restype is restype, prefix + name
    return seen


def test_prototypes_set_at_load_gpu_library():
    """In a fresh interpreter: gpu.lib() alone, no operator constructed."""
    import subprocess
    import sys
    code = (
        "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "from test_cabi import _assert_declared\n"
        "from arroyo_amd import gpu\n"
        "n = _assert_declared(gpu.lib(), 'arroyo_amd_', True)\n"
        "print('declared', n)\n" % (ROOT, os.path.join(ROOT, "tests")))
    _build()
    p = subprocess.run([sys.executable, "-c", code], capture_output=True,
                       text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip() == f"declared {len(SYMBOLS)}"


def test_prototypes_set_at_load_oracle_library():
    import subprocess
    import sys
    code = (
        "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "from test_cabi import _assert_declared\n"
        "import oracle\n"
        "n = _assert_declared(oracle.lib(), 'oracle_', False)\n"
        "print('declared', n)\n" % (ROOT, os.path.join(ROOT, "tests")))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True,
                       text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    # seven families: create, destroy, last_error, process_batch at least
    assert int(p.stdout.split()[1]) >= 7 * 4 + 1


# ---- the handle base ------------------------------------------------------

def test_oracle_updagg_constructs_and_gpu_only_call_names_symbol():
    import numpy as np

    import oracle
    from arroyo_amd import cabi as c
    op = oracle.make_updagg_op(c.make_updagg_config(
        [(c.COUNT, -1), (c.SUM, 0)], n_keys=1, n_value_cols=1))
    key = np.array([1, 2, 1], dtype=np.int64)
    val = np.array([10, 20, 30], dtype=np.int64)
    op.process_batch([key, val, np.zeros(3, dtype=np.int64)])
    out = op.flush()
    order = np.argsort(out[0])
    assert out[0][order].tolist() == [1, 2]
    assert out[1][order].tolist() == [2, 1]
    assert out[2][order].tolist() == [40, 20]
    with pytest.raises(AttributeError,
                       match="oracle_updagg_process_batch_device"):
        op.process_batch_device([], 0)
    op.close()


def _gpu_factories():
    from arroyo_amd import cabi as c
    from arroyo_amd import gpu
    return [
        (gpu.make_op, c.make_config(10**9, 10**9, [(c.COUNT, -1)])),
        (gpu.make_join_op, c.make_join_config()),
        (gpu.make_session_op, c.make_session_config(10**9, [(c.COUNT, -1)])),
        (gpu.make_expjoin_op, c.make_expjoin_config(10**9)),
        (gpu.make_updagg_op, c.make_updagg_config([(c.COUNT, -1)])),
        (gpu.make_windowfn_op, c.make_windowfn_config(2, 0, [(0, False)])),
        (gpu.make_map_op, c.make_map_config(1, [], [0])),
        (gpu.make_strkey, c.make_strkey_config()),
        (gpu.make_shuffler, c.make_shuffle_config(2, 1)),
    ]


def test_every_create_failure_reports_the_decoded_reason():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present; covered by -m gpu tests")
    factories = _gpu_factories()
    assert len(factories) == 9
    for make, cfg in factories:
        with pytest.raises(RuntimeError) as e:
            make(cfg)
        text = str(e.value)
        assert text.startswith("arroyo_amd_"), text
        assert "create failed: " in text and "b'" not in text, text
        assert text.split("create failed: ", 1)[1].strip(), text


def test_close_twice_and_fn_table_for_every_oracle_family():
    import oracle
    from arroyo_amd import cabi as c
    ops = [
        oracle.make_op(c.make_config(10**9, 10**9, [(c.COUNT, -1)])),
        oracle.make_join_op(c.make_join_config()),
        oracle.make_session_op(c.make_session_config(10**9,
                                                     [(c.COUNT, -1)])),
        oracle.make_expjoin_op(c.make_expjoin_config(10**9)),
        oracle.make_updagg_op(c.make_updagg_config([(c.COUNT, -1)])),
        oracle.make_windowfn_op(c.make_windowfn_config(2, 0, [(0, False)])),
        oracle.make_map_op(c.make_map_config(1, [], [0])),
    ]
    for op in ops:
        assert op._h
        assert "_lib_prefix" not in op._fn
        for name in ("create", "process_batch", "free_out", "destroy",
                     "last_error"):
            assert name in op._fn, (type(op).__name__, name)
        op.close()
        assert op._h is None
        op.close()
        assert op._h is None


def test_oracle_handle_watermarks_fallback():
    """WindowOp.handle_watermarks falls back to a sequential Python loop
    on libraries without the batched export (the oracle): emissions must
    equal per-watermark calls, concatenated."""
    import numpy as np

    import oracle
    from arroyo_amd import cabi as c

    def stream(op, batched):
        rng = np.random.default_rng(11)
        outs = []
        for i in range(6):
            ts = (1_600_000_000 * 10**9 +
                  np.arange(2000, dtype=np.int64) * 10**6 +
                  i * 2 * 10**9)
            key = rng.integers(0, 50, size=2000).astype(np.int64)
            op.process_batch([key, ts])
            wms = [int(ts[-1]) - 10**9]
            if batched:
                out = op.handle_watermarks(wms)
                if out and len(out[0]):
                    outs.append(out)
            else:
                for w in wms:
                    out = op.handle_watermark(w)
                    if out and len(out[0]):
                        outs.append(out)
        return outs

    cfg = lambda: c.make_config(width_ns=4 * 10**9, slide_ns=2 * 10**9,
                                n_keys=1, n_value_cols=0,
                                aggs=[(c.COUNT, -1)], log2_capacity=12)
    a = oracle.make_op(cfg())
    b = oracle.make_op(cfg())
    sa = stream(a, False)
    sb = stream(b, True)
    a.close()
    b.close()
    assert len(sa) == len(sb)
    for x, y in zip(sa, sb):
        for cx, cy in zip(x, y):
            assert np.array_equal(cx, cy)
