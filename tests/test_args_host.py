"""CPU: the host-only side of the argument list (include/stark_mi.h, "Argument list") -- smi_air_plan_args and its refusals,
the transcript layout, mirror.Air.add_permutation / add_lookup, and the declarations in the header, the loader and the Rust
binding."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import args_compose as agc
import ext_compose as xc
import perm_compose as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["smi_air_plan_args", "smi_dev_args_columns", "smi_dev_air_compose_args", "smi_dev_air_prove_args", "smi_air_verify_args"]
P, L = ("perm", [0], [1]), ("lookup", [2], [3], 4)


@pytest.fixture(scope="module")
def s():
    import stark_rs_amd
    stark_rs_amd.build()
    return stark_rs_amd


def raw_args(args, count=None):
    """-> a _lib.AirArgs of argument tuples, without the mirror's own refusals; a tuple's kind may be an integer"""
    from stark_rs_amd import _lib
    keep, raw = [], (_lib.AirArg * max(len(args), 1))()
    for a, arg in enumerate(args):
        la, ra = np.array(arg[1], dtype=np.uint32), np.array(arg[2], dtype=np.uint32)
        keep += [la, ra]
        kind = {"perm": 0, "lookup": 1}.get(arg[0], arg[0])
        raw[a] = _lib.AirArg(kind, len(la), arg[3] if len(arg) > 3 else 0, 0, la.ctypes.data_as(_lib.u32p), ra.ctypes.data_as(_lib.u32p))
    out = _lib.AirArgs(len(args) if count is None else count, 0, raw)
    out._keep = (keep, raw)
    return out


def plan(s, p, air, args, n_cols, log_n, lb):
    from stark_rs_amd import _lib, engine
    return engine.air_plan_args(p, air.flatten(p), args, _lib.StarkCfg(log_n, lb, n_cols, 1, 1, 3, 0, 1))


@pytest.mark.parametrize("p,g", xc.PRIMES)
def test_plan_takes_degree_two_or_three_by_the_mix(s, p, g):
    from stark_rs_amd.mirror import Air
    assert plan(s, p, Air(5), raw_args([P]), 5, 6, 2) == (2, 4)          # permutations alone: d = 2, D = 1, E = B
    assert plan(s, p, Air(5), raw_args([P, P]), 5, 6, 3) == (2, 8)
    assert plan(s, p, Air(5), raw_args([L]), 5, 6, 3) == (3, 4)          # any lookup: d = 3, D = 2, E = B / 2
    assert plan(s, p, Air(5), raw_args([P, L]), 5, 6, 3) == (3, 4)
    assert plan(s, p, Air(5), raw_args([L, P, L]), 5, 6, 4) == (3, 8)
    air, _cols = pm.cubic(64, p)                                         # the AIR's own degree 3 beside permutations
    air.n_cols = 5
    assert plan(s, p, air, raw_args([P]), 5, 6, 3) == (3, 4)
    for args in ([L], [P, L], [L, P], [P, P, L]):                        # log_blowup = 2 refuses any list with a lookup
        with pytest.raises(s.StarkMiError) as ei:
            plan(s, p, Air(5), raw_args(args), 5, 6, 2)
        assert ei.value.status == -10 and "2^log_blowup / D < 4" in str(ei.value)
    # the engine's dispatch and the restatement's plan agree
    air = agc.mirror_air(Air(5), [P, L])
    from stark_rs_amd import _lib, engine
    a = air.flatten(p)
    assert engine.air_plan_args(p, a, a.args, _lib.StarkCfg(6, 3, 5, 1, 1, 3, 0, 1)) == (3, 4) == (agc.plan(air, [P, L], 3)[0], agc.plan(air, [P, L], 3)[2])


@pytest.mark.parametrize("args,count,text", [
    ([], None, "count must be in 1 .. SMI_ARGS_MAX (8)"),
    ([P] * 8, 9, "count must be in 1 .. SMI_ARGS_MAX (8)"),
    ([P, ("perm", [], [])], None, "argument 1: perm: width must be in 1 .. SMI_PERM_MAX_WIDTH (8)"),
    ([("lookup", list(range(9)), list(range(9)), 4), P], None, "argument 0: lookup: width must be in 1 .. SMI_LOOKUP_MAX_WIDTH (8)"),
    ([P, L, ("perm", [0], [5])], None, "argument 2: perm: right_col must be < n_cols"),
    ([P, ("perm", [7], [0])], None, "argument 1: perm: left_col must be < n_cols"),
    ([L, ("lookup", [0], [9], 4)], None, "argument 1: lookup: table_col must be < n_cols"),
    ([P, P, P, ("lookup", [0], [1], 5)], None, "argument 3: lookup: mult_col must be < n_cols"),
    ([P, ("lookup", [0], [1], 1)], None, "argument 1: lookup: mult_col must be none of the tuple columns"),
    ([P, (2, [0], [1])], None, "argument 1: kind must be SMI_ARG_PERM (0) or SMI_ARG_LOOKUP (1)"),
])
def test_limits_name_the_argument(s, args, count, text):
    from stark_rs_amd.mirror import Air
    p, _g = xc.PRIMES[0]
    with pytest.raises(s.StarkMiError) as ei:
        plan(s, p, Air(5), raw_args(args, count), 5, 6, 3)
    assert ei.value.status == -50 and text in str(ei.value)


def test_eight_arguments_of_width_eight_are_planned(s):
    from stark_rs_amd.mirror import Air
    p, _g = xc.PRIMES[1]
    wide = [("perm", list(range(8)), list(range(8, 16))), ("lookup", list(range(8)), list(range(8, 16)), 16)] * 4
    assert plan(s, p, Air(17), raw_args(wide), 17, 6, 3) == (3, 4)


# ---------------------------------------------------------------------------------------------- the transcript
@pytest.fixture(scope="module")
def emu(s):
    from stark_rs_amd._lib import EMU_PATH
    lib = C.CDLL(EMU_PATH)
    lib.emu_args_transcript.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
    lib.emu_args_transcript.restype = C.c_uint64
    lib.emu_air_transcript.argtypes = [C.c_int, C.c_char_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    lib.emu_air_transcript.restype = C.c_uint64
    lib.emu_fs_seed.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_void_p]
    lib.emu_fs_seed.restype = None
    return lib


def args_transcript(emu, roots, W, K, A):
    n = 8 + 4 * (W + K + 2 * A)
    got, seed, length = np.zeros(n + 1, dtype=np.uint64), np.zeros(17, dtype=np.uint32), C.c_uint64()
    got[n] = 0x5a5a
    assert emu.emu_args_transcript(roots, W, K, A, got.ctypes.data, seed.ctypes.data, C.byref(length)) == n
    assert got[n] == 0x5a5a
    return [int(x) for x in got[:n]], list(seed), length.value


@pytest.mark.parametrize("W,K,A", [(1, 0, 1), (2, 1, 2), (3, 3, 3), (5, 2, 8)])
def test_transcript_length_and_challenges(oracle, emu, W, K, A):
    roots = np.random.default_rng(W + 10 * A).integers(0, 256, 64, dtype=np.uint8).tobytes()
    got, seed, length = args_transcript(emu, roots, W, K, A)
    assert length == 32 + 64 + 32 + 32 * (W + K + 2 * A) == agc.transcript_len(W, K, A)
    tr, ch = pm.challenges(oracle, roots[:32])
    tr, wts = pm.weights(oracle, tr, roots[32:], W + K + 2 * A)
    assert got == ch + wts and len(tr) == length
    words, phase = np.zeros(16, dtype=np.uint32), C.c_uint32(99)
    emu.emu_fs_seed(bytes(tr), len(tr), words.ctypes.data, C.addressof(phase))
    assert seed[:16] == list(words) and seed[16] == phase.value


@pytest.mark.parametrize("W,K", [(1, 0), (2, 1), (3, 3)])
def test_one_argument_gives_the_permutation_proofs_transcript(emu, W, K):
    roots = np.random.default_rng(7 * W + K).integers(0, 256, 64, dtype=np.uint8).tobytes()
    got, seed, _length = args_transcript(emu, roots, W, K, 1)
    n = 8 + 4 * (W + K + 2)
    want, wseed = np.zeros(n, dtype=np.uint64), np.zeros(17, dtype=np.uint32)
    assert emu.emu_air_transcript(3, roots, W, K, want.ctypes.data, wseed.ctypes.data) == n
    assert got == [int(x) for x in want] and seed == list(wseed)


# ---------------------------------------------------------------------------------------------- the mirror
def test_mirror_appends_arguments_and_flattens_them():
    from stark_rs_amd.mirror import Air
    p, _g = xc.PRIMES[0]
    air = Air(9).add_permutation([0, 1], [2, 3]).add_lookup([4], [5], 6).add_lookup([7], [5], 8)
    assert air.args == [("perm", [0, 1], [2, 3]), ("lookup", [4], [5], 6), ("lookup", [7], [5], 8)]
    flat = air.flatten(p)
    assert flat.perm is None and flat.lookup is None and flat.args.count == 3
    got = [(flat.args.arg[a].kind, flat.args.arg[a].width, flat.args.arg[a].mult_col, [flat.args.arg[a].a_col[j] for j in range(flat.args.arg[a].width)],
            [flat.args.arg[a].b_col[j] for j in range(flat.args.arg[a].width)]) for a in range(3)]
    assert got == [(0, 2, 0, [0, 1], [2, 3]), (1, 1, 6, [4], [5]), (1, 1, 8, [7], [5])]
    assert Air(3).flatten(p).args is None
    assert Air(3).permutation([0], [1]).flatten(p).args is None and Air(3).lookup([0], [1], 2).flatten(p).args is None


def test_mirror_refusals_name_the_argument():
    from stark_rs_amd.mirror import Air
    with pytest.raises(ValueError, match="argument 1: a permutation relates tuples of one width"):
        Air(4).add_lookup([0], [1], 2).add_permutation([0, 1], [2])
    with pytest.raises(ValueError, match="argument 0: a lookup relates tuples of one width"):
        Air(4).add_lookup([0], [1, 2], 3)
    with pytest.raises(ValueError, match="argument 2: 1 .. 8 columns a side"):
        Air(4).add_permutation([0], [1]).add_permutation([0], [1]).add_permutation([], [])
    air = Air(4)
    for _ in range(8):
        air.add_permutation([0], [1])
    with pytest.raises(ValueError, match="argument 8: an argument list holds at most 8 arguments"):
        air.add_lookup([0], [1], 2)
    # mixing with permutation() / lookup() is refused in either order
    with pytest.raises(ValueError, match="argument 0: an argument list does not mix with permutation"):
        Air(4).permutation([0], [1]).add_lookup([0], [1], 2)
    with pytest.raises(ValueError, match="argument 0: an argument list does not mix with permutation"):
        Air(4).lookup([0], [1], 2).add_permutation([0], [1])
    with pytest.raises(ValueError, match="permutation\\(\\) does not mix with an argument list"):
        Air(4).add_permutation([0], [1]).permutation([0], [1])
    with pytest.raises(ValueError, match="lookup\\(\\) does not mix with an argument list"):
        Air(4).add_permutation([0], [1]).lookup([0], [1], 2)
    # the existing refusals keep their words
    with pytest.raises(ValueError, match="one permutation per AIR"):
        Air(4).permutation([0], [1]).permutation([0], [1])
    with pytest.raises(ValueError, match="an AIR takes a permutation or a lookup, not both"):
        Air(4).permutation([0], [1]).lookup([0], [1], 2)


# ---------------------------------------------------------------------------------------------- the declarations
def test_header_loader_and_rust_declare_the_entry_points_and_structs(s):
    from stark_rs_amd import _lib
    header = open(os.path.join(ROOT, "include", "stark_mi.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "stark_mi.rs")).read()
    names = s.declared_symbols()
    lib = C.CDLL(s.build())
    for name in ENTRY_POINTS:
        assert name in names and hasattr(lib, name) and f"pub fn {name}(" in rust, name
    assert "#define SMI_ARGS_MAX 8" in header and "pub const SMI_ARGS_MAX: u32 = 8;" in rust
    assert "pub const SMI_ARG_PERM: u32 = 0;" in rust and "pub const SMI_ARG_LOOKUP: u32 = 1;" in rust
    assert C.sizeof(_lib.AirArg) == 32 and C.sizeof(_lib.AirArgs) == 16
    body = re.search(r"typedef struct smi_air_arg \{(.*?)\} smi_air_arg;", re.sub(r"/\*.*?\*/", "", header, flags=re.S), flags=re.S).group(1)
    assert re.findall(r"(\w+);", body) == [f[0] for f in _lib.AirArg._fields_] == re.findall(r"pub (\w+):", re.search(r"pub struct smi_air_arg \{(.*?)\n\}", rust, flags=re.S).group(1))
    body = re.search(r"typedef struct smi_air_args \{(.*?)\} smi_air_args;", re.sub(r"/\*.*?\*/", "", header, flags=re.S), flags=re.S).group(1)
    assert re.findall(r"(\w+);", body) == [f[0] for f in _lib.AirArgs._fields_] == re.findall(r"pub (\w+):", re.search(r"pub struct smi_air_args \{(.*?)\n\}", rust, flags=re.S).group(1))
    # the section sits between the lookup argument and the multi-GPU part, and the pinned sentences stand
    assert header.index("---- Lookup argument") < header.index("---- Argument list") < header.index("---- multi-GPU")
    assert "one permutation per proof" in header and "One lookup per\n *   proof, and not together with a permutation" in header
    for wrapper in ("pub fn plan_args", "pub fn prove_args", "pub fn verify_args", "pub fn compose_args", "pub struct Arguments"):
        assert wrapper in rust[rust.index("// END GENERATED"):], wrapper
    # the verifier's sentences live beside the lane code, where the recorded verdict fixture does not look for them
    core = open(os.path.join(ROOT, "stark_rs_amd", "csrc", "args_core.h")).read()
    assert core.count('"argument openings: ') == 6 and "argument openings" not in open(os.path.join(ROOT, "stark_rs_amd", "csrc", "verify.hip")).read()


def test_engine_refuses_an_argument_list_without_row_leaves_and_ext(s):
    """host-side checks of the Engine's dispatch that need no device: a stand-in object carries the methods' self"""
    from stark_rs_amd.engine import Engine
    from stark_rs_amd.mirror import Air
    eng = Engine.__new__(Engine)
    eng.p = xc.PRIMES[0][0]
    air = Air(5).add_permutation([0], [1])
    for kw in (dict(), dict(row_leaves=True), dict(ext=True)):
        with pytest.raises(ValueError, match="argument list needs row_leaves=True, ext=True"):
            eng.dev_air_prove(air, 0, 5, 4, 3, 2, **kw)
        with pytest.raises(ValueError, match="argument list needs row_leaves=True, ext=True"):
            eng.air_verify(air, b"", [bytes(32), bytes(32)], 5, 4, 3, 2, **kw)
    with pytest.raises(ValueError, match="no argument list"):
        eng.dev_args_columns(Air(5), 0, 5, 4, [0] * 8, 0)
    with pytest.raises(ValueError, match="the argument list has no lookup"):
        eng.dev_air_prove(air, 0, 5, 4, 3, 2, row_leaves=True, ext=True, fill_multiplicities=True)
