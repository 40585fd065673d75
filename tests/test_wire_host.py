"""The wire code (otti_amd/csrc/wire.h, wire.cpp) on the host: tests/wire_check.cpp — own main, host sources only, built with the address and
undefined-behaviour sanitizers (their runtime linked into the program: nothing is added to LD_PRELOAD and the environment is passed on as it is) —
parses and re-serialises proofs and commitments made by the CPU oracle: NIZK proofs at n = 2, 64 and 1000, SNARK proofs and their commitments at
n = 2, 16 and 200 (n = 2: every vector at its shortest, no reduction round where lgR = 0).  serialize(parse(b)) == b byte for byte; EVERY proper
prefix of every file, and every file with a byte appended, is refused as malformed (-12) with no read past the buffer; and each count set to its
bound + 1, one file per counted vector of every object, is refused as malformed before anything is allocated for it.  Where the counts sit comes
from the independent field map of proof_fields.py; the bounds are written out below."""
import os
import re
import subprocess

import host_build
import otti_amd as oa
import proof_fields as pf
import proof_fields_cases as pc

FIXED_3 = re.compile(r"^(eval_(row|col)\.(read|write)|dotp_(left|right)|h_\w+|proof_(mem|ops)\.layers\[\]\.coeffs\[\])\.len$")   # arrays of three


def bound(group):
    """the largest count the reader accepts for a counted vector, by its struct member"""
    if group == "comm_vars.len":
        return 1 << 20
    if group in ("comm_derefs.len", "comm_ops.len", "comm_mem.len"):
        return 1 << 24
    if group.endswith(".proofs[].z.len"):
        return 4
    return 3 if FIXED_3.match(group) else 64


def test_bounds_by_member():
    assert [bound(g) for g in ("sc1.comm_polys.len", "sc2.proofs.len", "sc1.proofs[].z.len", "polyeval.L.len", "rx.len", "proof_ops.layers.len",
                               "proof_ops.layers[].coeffs.len", "proof_ops.layers[].coeffs[].len", "proof_mem.layers[].left.len", "proof_ops.dotp_left.len",
                               "dotp_left.len", "eval_col.write.len", "h_deref_col.len", "pe_mem.R.len")] == [64, 64, 4, 64, 64, 64, 64, 3, 64, 64, 3, 3, 3, 64]


def _past_bound(blob, fields):
    """[(member, bytes)]: for each counted vector of the object (the first of its kind), the blob with that count set to its bound + 1"""
    out, seen = [], set()
    for name, off, kind in fields:
        g = pf.group(name)
        if kind == "len" and g not in seen:
            seen.add(g)
            out.append((g, blob[:off] + (bound(g) + 1).to_bytes(8, "little") + blob[off + 8:]))
    return out


def test_round_trip_prefixes_and_counts_past_their_bounds(tmp_path):
    exe = host_build.build_check(tmp_path, "wire_check.cpp", "wire_check", host_build.ASAN_UBSAN)
    files = []
    for n in (2, 64, 1000):
        files.append(("nizk", "nizk%d" % n, pc.NizkCase(oa.synth_r1cs(n, 3 if n > 2 else 1, 7)).oracle_proof(), pf.nizk))
    for n in (2, 16, 200):
        case = pc.SnarkCase(oa.synth_r1cs(n, 3 if n > 2 else 1, 7))
        files.append(("snark", "snark%d" % n, case.oracle_proof(), pf.snark))
        files.append(("comm", "comm%d" % n, case.comm_bytes, pf.commitment))
    lines, prefixes, members = [], 0, set()
    for kind, name, blob, fields in files:
        (tmp_path / name).write_bytes(blob)
        lines.append("roundtrip %s %s" % (kind, tmp_path / name))
        prefixes += len(blob)
        if name in ("nizk64", "snark16", "comm16"):
            for k, (g, mutant) in enumerate(_past_bound(blob, fields(blob))):
                (tmp_path / ("%s.count%d" % (name, k))).write_bytes(mutant)
                lines.append("refuse %s %s" % (kind, tmp_path / ("%s.count%d" % (name, k))))
                members.add((kind, g))
    # every counted member of the three objects: 13 of a NIZK proof (rx and ry among them), the 11 of its R1CSProof and 36 more of a SNARK proof,
    # 2 of a commitment
    assert len(members) == 13 + 47 + 2, sorted(members)
    manifest = tmp_path / "manifest.txt"
    manifest.write_text("\n".join(lines) + "\n")
    r = subprocess.run([str(exe), str(manifest)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    tail = r.stdout[-3000:] + r.stderr[-3000:]
    assert r.returncode == 0, tail
    assert "wire_check: %d files, %d prefixes, %d counts past their bound refused, 0 failures" % (len(lines), prefixes, len(members)) in r.stdout, tail
