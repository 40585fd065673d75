"""The .zkif files both ingest suites feed their readers (tests/test_zkif_walk_host.py: the walker on the host under sanitizers;
tests/test_gpu_zkif_ingest.py: the kernels): triples the product's writer makes, official-layout files from fb_reverse_builder — shapes the
product's writer never produces —, files with exactly one defect each, and seeded mutants of one small circuit.  Everything is a function of its
arguments and a fixed seed: the GPU suite's first 200 mutants are byte for byte the ones the sanitizer run has walked.  Test infrastructure only."""
import os
import random
import struct

import numpy as np

import otti_amd as oa
import fb_reverse_builder as fb

L = 2 ** 252 + 27742317777372353535851937790883648493


def product_triple(dirpath, name, n, ni, compiler=False, seed=1):
    """a synthetic instance written by the product's writer; returns (paths, r1cs dict)"""
    r = (oa.synth_r1cs_compiler_like if compiler else oa.synth_r1cs)(n, ni, seed)
    paths = tuple(os.path.join(dirpath, name + ext) for ext in (".zkif", ".inp.zkif", ".wit.zkif"))
    oa.zkif_write(r, *paths)
    return paths, r


# ---- official layout.  One tiny satisfiable system: id 0 = one, id 1 = the input x = 3, ids 2, 3 = the witness w1 = 3, w2 = 9
ROW_SQUARE = ([(2, 1)], [(2, 1)], [(3, 1)])                      # w1 * w1 = w2
ROW_INPUT = ([(1, 1)], [(0, 1)], [(2, 1)])                       # x * 1 = w1


def _lc(B, lc, width):
    """lc: None (no table) | list of (id, coefficient) | dict(ids=[..], values=bytes or None)"""
    if lc is None:
        return None
    if isinstance(lc, dict):
        voff = B.vector_bytes(lc["values"]) if lc["values"] is not None else None
        ioff = B.vector_u64(lc["ids"])
        f = {0: ("offset", ioff)}
        if voff is not None:
            f[1] = ("offset", voff)
        return B.table(3, f)
    return fb._variables(B, [i for i, _ in lc], [v for _, v in lc], width)


def cs_message(rows, width=32):
    B = fb.Builder()
    offs = []
    for lcs in rows:
        sub = [_lc(B, lc, width) for lc in reversed(lcs)][::-1]
        offs.append(B.table(3, {k: ("offset", sub[k]) for k in range(3) if sub[k] is not None}))
    vec = B.vector_offsets(offs)
    cs = B.table(2, {0: ("offset", vec)})
    root = B.table(2, {0: ("u8", 2), 1: ("offset", cs)})
    return B.finish_size_prefixed(root)


def aliased_message(n_slots, ids, coefficients):
    """a ConstraintSystem whose n_slots constraint offsets ALL point at one BilinearConstraint table, whose three combinations all point at one
    Variables table: valid FlatBuffers (offsets only have to point forward), entries far beyond what the bytes could hold one by one.  Laid out
    forward by hand — the builder prepends, which is quadratic in a vector of 2^19 offsets."""
    b = bytearray(struct.pack("<I4s", 16, b"zkif"))
    b += struct.pack("<HHHH", 8, 12, 8, 4)                      # root vtable at 8: type at +8, message at +4
    b += struct.pack("<iIB3x", 8, 0, 2)                         # root table at 16 (message offset patched below), type 2
    b += struct.pack("<HHH2x", 6, 8, 4)                         # ConstraintSystem vtable at 28
    cs = len(b)
    b += struct.pack("<iI", cs - 28, 4)                         # its table at 36: constraints vector right behind
    struct.pack_into("<I", b, 20, cs - 20)
    vec = len(b)
    b += struct.pack("<I", n_slots) + bytes(4 * n_slots)
    vt = len(b)
    b += struct.pack("<HHHHH2x", 10, 16, 4, 8, 12)              # BilinearConstraint vtable
    bc = len(b)
    b += struct.pack("<i", bc - vt) + bytes(12)
    vvt = len(b)
    b += struct.pack("<HHHH", 8, 12, 4, 8)                      # Variables vtable
    var = len(b)
    b += struct.pack("<i", var - vvt) + bytes(8)
    idv = len(b)
    b += struct.pack("<I", len(ids)) + b"".join(struct.pack("<Q", i) for i in ids)
    vals = len(b)
    b += struct.pack("<I", 32 * len(ids)) + b"".join(int(c).to_bytes(32, "little") for c in coefficients)
    b += bytes(-len(b) % 8)
    struct.pack_into("<II", b, var + 4, idv - (var + 4), vals - (var + 8))
    for k in range(3):
        struct.pack_into("<I", b, bc + 4 + 4 * k, var - (bc + 4 + 4 * k))
    slots = (bc - (vec + 4) - 4 * np.arange(n_slots, dtype=np.int64)).astype("<u4")
    b[vec + 4:vec + 4 + 4 * n_slots] = slots.tobytes()
    return struct.pack("<I", len(b)) + bytes(b)


def too_many_entries():
    """2^19 constraints that share one table of 2^13 ids: 2^32 entries per matrix from 2.4 MB.  The device ingest refuses (its counts are 32-bit);
    the host loader would need 200 GB for the lists, so nothing compares the two on this one."""
    return header() + aliased_message(1 << 19, [0] * (1 << 13), [1] * (1 << 13))


def command_message():
    B = fb.Builder()
    cmd = B.table(3, {0: ("u8", 1)})
    root = B.table(2, {0: ("u8", 4), 1: ("offset", cmd)})
    return B.finish_size_prefixed(root)


def header(values=None):
    return fb.circuit_header([1], values, 4, L - 1)


INPUTS = header([3])
WITNESS = fb.witness([2, 3], [3, 9])


def write_case(dirpath, name, circuit):
    """a case is its circuit file; inputs and witness are the tiny system's"""
    paths = tuple(os.path.join(dirpath, name + ext) for ext in (".zkif", ".inp.zkif", ".wit.zkif"))
    for p, data in zip(paths, (circuit, INPUTS, WITNESS)):
        with open(p, "wb") as f:
            f.write(data)
    return paths


def shaped_cases():
    """(name, circuit bytes): layouts both loaders accept"""
    rows = [ROW_SQUARE, ROW_INPUT, ROW_SQUARE]
    out = [(f"width{w}", header() + cs_message(rows, w)) for w in (1, 8, 31, 33)]
    out.append(("absent_table", header() + cs_message([ROW_SQUARE, ([(2, 1)], None, [(3, 1)]), ROW_INPUT])))
    out.append(("zero_ids", header() + cs_message([ROW_SQUARE, ([(2, 1)], [], [(3, 1)]), ROW_INPUT])))
    out.append(("empty_message", header() + cs_message([ROW_SQUARE]) + cs_message([]) + cs_message([ROW_INPUT])))
    out.append(("no_constraints", header() + cs_message([])))
    out.append(("one_constraint", header() + cs_message([ROW_SQUARE])))
    out.append(("five_messages", header() + b"".join(cs_message([ROW_INPUT if i % 2 else ROW_SQUARE for i in range(n)]) for n in (1, 2, 3, 64, 65))))
    out.append(("header_and_command_between", header() + cs_message(rows) + header() + command_message() + cs_message(rows)))
    out.append(("misaligned_ids", _misaligned(header(), cs_message(rows))))
    out.append(("aliased_tables", header() + aliased_message(5, [0, 2, 3], [1, 3, L - 1])))     # 5 rows x 3 entries per matrix from one table
    return out


# ---- a reader just good enough to find what a defect patches (positions within a message BODY, i.e. behind its size prefix)
def _u32(b, o):
    return struct.unpack_from("<I", b, o)[0]


def _field(b, pos, k):
    vt = pos - struct.unpack_from("<i", b, pos)[0]
    vsize = struct.unpack_from("<H", b, vt)[0]
    if 4 + 2 * k + 2 > vsize:
        return 0
    off = struct.unpack_from("<H", b, vt + 4 + 2 * k)[0]
    return pos + off if off else 0


def locate(body, row=0, k=0):
    root = _u32(body, 0)
    f = _field(body, root, 1)
    cs = f + _u32(body, f)
    f = _field(body, cs, 0)
    vec = f + _u32(body, f)
    slot = vec + 4 + 4 * row
    bc = slot + _u32(body, slot)
    f = _field(body, bc, k)
    var = f + _u32(body, f)
    fi = _field(body, var, 0)
    ids = fi + _u32(body, fi)
    fv = _field(body, var, 1)
    vals = fv + _u32(body, fv) if fv else 0
    return dict(vec=vec, slot=slot, bc=bc, vars=var, ids_field=fi, ids=ids, vals=vals)


def _patched(head, msg, edit):
    body = bytearray(msg[4:])
    edit(body, locate(body))
    return head + struct.pack("<I", len(body)) + bytes(body)


def _misaligned(head, msg):
    """constraint 0's A ids vector moved to an ODD offset at the end of the message: in bounds, and no load of it is aligned"""
    def edit(body, at):
        body.extend(b"\0" * (1 if len(body) % 2 == 0 else 2))
        new = len(body)
        body.extend(struct.pack("<IQ", 1, 2))
        struct.pack_into("<I", body, at["ids_field"], new - at["ids_field"])
    return _patched(head, msg, edit)


def defect_cases():
    """(name, circuit bytes): exactly one defect each; both loaders refuse, with the same code"""
    rows = [ROW_SQUARE, ROW_INPUT, ROW_SQUARE]
    head, msg = header(), cs_message(rows)
    good = head + msg
    out = [("truncated", good[:-10])]
    out.append(("prefix_beyond_file", head + struct.pack("<I", len(msg) + 100) + msg[4:]))
    out.append(("missing_identifier", head + msg[:8] + b"zkiX" + msg[12:]))
    out.append(("trailing_bytes", good + b"\1\2\3"))
    out.append(("constraint_offset_beyond", _patched(head, msg, lambda b, at: struct.pack_into("<I", b, at["slot"], 0x7fffffff))))
    out.append(("vtable_before_start", _patched(head, msg, lambda b, at: struct.pack_into("<i", b, at["bc"], at["bc"] + 100))))
    out.append(("ids_count_beyond", _patched(head, msg, lambda b, at: struct.pack_into("<I", b, at["ids"], 0x10000000))))
    out.append(("values_not_multiple", head + cs_message([ROW_SQUARE, (dict(ids=[2, 3], values=bytes(33)), [(2, 1)], [(3, 1)])])))
    out.append(("ids_without_values", head + cs_message([ROW_SQUARE, (dict(ids=[2], values=None), [(2, 1)], [(3, 1)])])))
    out.append(("width33_nonzero_tail", head + cs_message([ROW_SQUARE, (dict(ids=[2], values=bytes([1] + [0] * 31 + [5])), [(2, 1)], [(3, 1)])])))
    out.append(("undeclared_id", head + cs_message([ROW_SQUARE, ([(999, 1)], [(2, 1)], [(3, 1)])])))
    out.append(("coefficient_l", head + cs_message([ROW_SQUARE, ([(2, 1)], [(2, L)], [(3, 1)])])))
    return out


# ---- seeded mutants of one circuit file: bytes, lengths, offsets
def mutants(circuit, n, seed=20260101):
    rng = random.Random(seed)
    extremes = (0, 1, 4, 8, 0x7fffffff, 0x80000000, 0xffffffff, 0xfffffff8)
    out = []
    for _ in range(n):
        b = bytearray(circuit)
        kind = rng.randrange(6)
        if kind == 0:                                            # truncate
            del b[rng.randrange(len(b)):]
        elif kind == 1:                                          # flip a few bits
            for _ in range(1 + rng.randrange(5)):
                b[rng.randrange(len(b))] ^= 1 << rng.randrange(8)
        elif kind == 2:                                          # an extreme word anywhere
            struct.pack_into("<I", b, rng.randrange(len(b) - 4), rng.choice(extremes))
        elif kind == 3:                                          # an aligned word (offsets, counts, vtable distances) nudged or made extreme
            o = 4 * rng.randrange(len(b) // 4)
            v = _u32(b, o)
            struct.pack_into("<I", b, o, rng.choice(extremes) if rng.randrange(3) == 0 else (v + rng.choice((-9, -4, -1, 1, 2, 4, 7, 33, 1 << 16))) & 0xffffffff)
        elif kind == 4:                                          # a 16-bit field (vtable sizes and slots)
            o = 2 * rng.randrange(len(b) // 2)
            struct.pack_into("<H", b, o, rng.choice((0, 2, 4, 6, 10, 0xffff, struct.unpack_from("<H", b, o)[0] + 2 & 0xffff)))
        else:                                                    # bytes appended
            b.extend(rng.randbytes(1 + rng.randrange(64)))
        out.append(bytes(b))
    return out
