"""The .inp.zkif / .wit.zkif files both witness-ingest suites feed their readers (tests/test_zkif_wit_walk_host.py: the reader on the host under
sanitizers; tests/test_gpu_witness_from_zkif.py: the kernel): official-layout files in shapes the product's writer never produces — element
widths, id orders, interleaved instance ids, the witness split over several messages with other messages in between —, files with exactly one
defect each, files with two defects of adjacent steps of the host pair's order, and seeded mutants of one witness file.  Every case comes with a
circuit file that declares the same ids, so that zkif_load on the three files is the reference.  Everything is a function of its arguments and a
fixed seed: the GPU suite's first 200 mutants are byte for byte the ones the sanitizer run has walked.  Test infrastructure only."""
import os
import random
import struct

import numpy as np

import fb_reverse_builder as fb
import zkif_ingest_cases as zc

L = zc.L
IO, INVALID_SCALAR, INVALID_INDEX, BAD_ARG = -22, -5, -6, -21
SPECIALS = (0, 1, 2 ** 64 - 1, 2 ** 64, L - 1)


def unknown_message():
    """a message whose root names a union member the schema does not have"""
    B = fb.Builder()
    t = B.table(1, {0: ("u8", 7)})
    root = B.table(2, {0: ("u8", 9), 1: ("offset", t)})
    return B.finish_size_prefixed(root)


def witness_raw(ids, values):
    """a Witness message whose values vector is the given bytes (None: no values field)"""
    B = fb.Builder()
    voff = B.vector_bytes(values) if values is not None else None
    ioff = B.vector_u64(ids)
    f = {0: ("offset", ioff)}
    if voff is not None:
        f[1] = ("offset", voff)
    av = B.table(3, f)
    w = B.table(1, {0: ("offset", av)})
    root = B.table(2, {0: ("u8", 3), 1: ("offset", w)})
    return B.finish_size_prefixed(root)


def circuit_for(inst_ids, free_id):
    """a circuit that declares the ids and constrains nothing of them: 1 * 1 = 1"""
    return fb.circuit_header(inst_ids, None, free_id, L - 1) + zc.cs_message([([(0, 1)], [(0, 1)], [(0, 1)])])


def _inst_ids(nv, ni, interleaved):
    """ni instance ids among the nv + ni ids 1 .. nv + ni: the first ni, or spread evenly among the witness ids and listed descending (the inputs' order
    is the header's list's, not the ids')"""
    total = nv + ni
    if not interleaved:
        return list(range(1, ni + 1)), total + 1
    return [1 + (k * total + total // 2) // ni for k in range(ni)][::-1], total + 1


def assignment(nv, ni=3, interleaved=True, width=32, order="ascending", splits=1, between=False, seed=7):
    """dict(circuit, inputs, witness: file bytes; vars: the (nv, 32) assignment zkif_load must give; inst_ids, free_id, pieces: the Witness messages' (ids, values))"""
    rng = random.Random(seed * 1000003 + nv * 31 + width)
    inst_ids, free_id = _inst_ids(nv, ni, interleaved) if ni else ([], nv + 1)
    inst = set(inst_ids)
    wit_ids = [i for i in range(1, free_id) if i not in inst]
    assert len(wit_ids) == nv
    bound = min(L, 2 ** (8 * width))
    vals = {i: rng.randrange(bound) if rng.randrange(4) else rng.randrange(min(bound, 2 ** 64)) for i in wit_ids}
    for k, s in enumerate(SPECIALS):                                 # the special values, where the width holds them, spread over the list
        if s < bound and nv:
            vals[wit_ids[(k * 13 + nv // 2) % nv]] = s
    listed = list(wit_ids)
    if order == "descending":
        listed.reverse()
    elif order == "shuffled":
        rng.shuffle(listed)
    cuts = sorted(rng.sample(range(nv + 1), splits - 1)) if splits > 1 and nv >= splits else [0] * (splits - 1)
    if splits == 5:
        cuts[2] = cuts[1]                                            # one of the five messages is empty
    pieces, at = [], 0
    for c in cuts + [nv]:
        pieces.append(listed[at:c]); at = c
    msgs = [fb.witness(p, [vals[i] for i in p], width) for p in pieces]
    if between and len(msgs) > 1:
        msgs[1:1] = [zc.command_message(), unknown_message()]
    cols = {i: k for k, i in enumerate(wit_ids)}
    vars32 = np.zeros((nv, 32), dtype=np.uint8)
    for i in wit_ids:
        vars32[cols[i]] = np.frombuffer(vals[i].to_bytes(32, "little"), dtype=np.uint8)
    in_vals = [rng.randrange(L) for _ in inst_ids]
    return dict(circuit=circuit_for(inst_ids, free_id), inputs=fb.circuit_header(inst_ids, in_vals, free_id, L - 1), witness=b"".join(msgs), vars=vars32,
                inst_ids=inst_ids, free_id=free_id, pieces=[(p, [vals[i] for i in p]) for p in pieces], input_values=in_vals)


def accepted_cases():
    """(name, assignment dict): shapes both paths accept"""
    out = []
    orders, splits = ("ascending", "descending", "shuffled"), (1, 2, 5)
    for k, nv in enumerate((1, 2, 31, 32, 33, 63, 64, 65, 1000, 5000)):          # bitmap word edges, more than one block
        ni = 0 if k % 3 == 1 else 3
        out.append((f"nv{nv}", assignment(nv, ni, True, 32, orders[k % 3], splits[(k + 1) % 3] if nv >= 5 else 1, between=nv == 64)))
    for w in (1, 8, 31, 33, 40):                                                 # 31 and 33 misalign every value
        out.append((f"width{w}", assignment(65, 2, True, w, "shuffled", 2)))
    out.append(("five_messages_between", assignment(300, 4, True, 32, "shuffled", 5, between=True)))
    out.append(("inputs_first_ids", assignment(40, 3, False, 32, "descending", 1)))
    return out


# ---- a reader just good enough to find what a defect patches (positions within a Witness message BODY)
def locate(body):
    root = zc._u32(body, 0)
    f = zc._field(body, root, 1)
    w = f + zc._u32(body, f)
    f = zc._field(body, w, 0)
    var = f + zc._u32(body, f)
    fi = zc._field(body, var, 0)
    ids = fi + zc._u32(body, fi)
    fv = zc._field(body, var, 1)
    vals = fv + zc._u32(body, fv) if fv else 0
    return dict(ids=ids, vals=vals)


def _patched(msg, edit):
    body = bytearray(msg[4:])
    edit(body, locate(body))
    return struct.pack("<I", len(body)) + bytes(body)


BASE_INST, BASE_FREE = [3], 8                                        # ids 1, 2, 4, 5, 6, 7 are the witness: six variables, one input
BASE_IDS = [1, 2, 4, 5, 6, 7]
BASE_VALS = [5, 2 ** 64, 0, L - 1, 9, 1]


def _base_inputs(value=11, inst=None, free_id=BASE_FREE):
    return fb.circuit_header(BASE_INST if inst is None else inst, [value] * len(BASE_INST if inst is None else inst), free_id, L - 1)


def _case(witness, inputs=None, circuit=None):
    return dict(circuit=circuit or circuit_for(BASE_INST, BASE_FREE), inputs=inputs or _base_inputs(), witness=witness)


def _wide(ids, vals, bad_at=None):
    """width 33: zero tails, except element bad_at"""
    b = b"".join(v.to_bytes(32, "little") + (b"\5" if k == bad_at else b"\0") for k, v in enumerate(vals))
    return witness_raw(ids, b)


def defect_cases():
    """(name, case dict, code): exactly one defect each; the host pair and the device path refuse, with this code"""
    good = fb.witness(BASE_IDS, BASE_VALS)
    out = [("truncated", _case(good[:-10]), IO)]
    out.append(("ids_count_beyond", _case(_patched(good, lambda b, at: struct.pack_into("<I", b, at["ids"], 0x10000000))), IO))
    out.append(("values_not_multiple", _case(witness_raw(BASE_IDS, bytes(32 * 6 + 1))), IO))
    out.append(("no_values", _case(witness_raw(BASE_IDS, None)), IO))
    out.append(("width33_nonzero_tail", _case(_wide(BASE_IDS, BASE_VALS, 4)), INVALID_SCALAR))
    out.append(("id_zero", _case(fb.witness([1, 2, 4, 0, 6, 7], BASE_VALS)), INVALID_INDEX))
    out.append(("instance_id", _case(fb.witness([1, 2, 4, 3, 6, 7], BASE_VALS)), INVALID_INDEX))
    out.append(("duplicate_id", _case(fb.witness([1, 2, 4, 5, 6, 6], BASE_VALS)), IO))
    out.append(("one_id_too_few", _case(fb.witness(BASE_IDS[:-2] + BASE_IDS[-1:], BASE_VALS[:-1])), IO))
    out.append(("value_l", _case(fb.witness(BASE_IDS, [5, 2, L, 1, 9, 1])), INVALID_SCALAR))
    out.append(("value_all_ones", _case(fb.witness(BASE_IDS, [5, 2, 0, 1, 9, 2 ** 256 - 1])), INVALID_SCALAR))
    out.append(("input_l", _case(good, _base_inputs(L)), INVALID_SCALAR))
    # a consistent pair of files for an instance of seven variables, beside the circuit of six
    out.append(("other_dimensions", _case(fb.witness(BASE_IDS + [8], BASE_VALS + [3]), _base_inputs(free_id=9)), BAD_ARG))
    return out


def two_defect_cases():
    """(name, case dict, code): two defects of adjacent steps of the host pair's order; the earlier step's code, wherever its defect sits in the file"""
    a_ids, a_vals, b_ids, b_vals = BASE_IDS[:3], BASE_VALS[:3], BASE_IDS[3:], BASE_VALS[3:]
    out = []
    # step 1 within itself: messages in file order, tables before tails
    out.append(("tail_then_broken_message", _case(_wide(a_ids, a_vals, 2) + fb.witness(b_ids, b_vals)[:-10]), INVALID_SCALAR))
    out.append(("broken_message_then_tail", _case(_patched(fb.witness(a_ids, a_vals), lambda b, at: struct.pack_into("<I", b, at["ids"], 0x10000000)) + _wide(b_ids, b_vals, 0)), IO))
    # 1 before 2: a tail in the LAST message, and one id too few
    out.append(("tail_and_count", _case(fb.witness(a_ids, a_vals) + _wide(b_ids[:-1], b_vals[:-1], 1)), INVALID_SCALAR))
    # 2 before 3: an instance id 0 in the inputs header (the id map's own code), and a message without values
    zero_inst = fb.circuit_header([0], [11], BASE_FREE + 1, L - 1)
    out.append(("instance_zero_and_no_values", _case(witness_raw(BASE_IDS + [3], None), zero_inst, circuit_for([0], BASE_FREE + 1)), INVALID_INDEX))
    # 3 before 4: a message without values behind one that assigns id 0
    out.append(("no_values_and_id_zero", _case(fb.witness([0, 2, 4], a_vals) + witness_raw(b_ids, None)), IO))
    # 4 before 5: a variable assigned twice FIRST in the list, an instance id last
    out.append(("instance_id_and_duplicate", _case(fb.witness([1, 1, 4], a_vals) + fb.witness([5, 6, 3], b_vals)), INVALID_INDEX))
    # 5 before 6: a value l first in the list, a variable assigned twice last
    out.append(("duplicate_and_value_l", _case(fb.witness(a_ids, [L, 2, 0]) + fb.witness([5, 6, 6], b_vals)), IO))
    return out


def write_case(dirpath, name, case):
    paths = tuple(os.path.join(dirpath, name + ext) for ext in (".zkif", ".inp.zkif", ".wit.zkif"))
    for p, key in zip(paths, ("circuit", "inputs", "witness")):
        with open(p, "wb") as f:
            f.write(case[key])
    return paths


def mutant_base():
    """the witness file the mutants are made of: three messages of width 33, other messages in between, beside an interleaved instance id"""
    a = assignment(48, 3, True, 33, "shuffled", 3, between=True, seed=11)
    return a


def mutants(witness, n, seed=20260202):
    return zc.mutants(witness, n, seed)
