"""A proof's field map and its substitutes: where every point, scalar and vector count of a NIZK proof, a SNARK proof and a computation commitment
sits in the wire form, and the one-field-at-a-time replacements the verifier tests apply there.  Pure Python: no library, no GPU.

The wire forms are bincode, as the product's own writers emit them (NizkProof::serialize, SnarkProof::serialize and CompComm::serialize in
wire.cpp): a vector is a u64 count followed by its elements, a point is its 32-byte ristretto255 encoding, a scalar the
32 bytes of its Montgomery limbs (x * 2^256 mod l), little endian.  nizk(b), snark(b) and commitment(b) return [(name, offset, kind)] in wire
order, kind in "pt", "fr", "len" (a vector's count) and, in a commitment only, "u64" (its six dimensions); each walk must end at len(b).  Names
follow the structs: sc1.proofs[3].z[2], prod.delta, polyeval.L[0], proof_ops.layers[2].coeffs[1][0], h_row_read_ts[1], pe_mem.z2; a vector's count
is <vector>.len.

Substitutes, each changing one field and nothing else:
    pt   identity      32 zero bytes: a valid encoding
         other_point   the bytes of the next point field of the same blob that differ from this one and from zero: it decodes, so only an
                       equation or the transcript can refuse it
         undecodable   01 00 .. 00 (s = 1 is odd)
    fr   plus_one      (raw + 1) mod l
         zero
         plus_l        raw + l: below 2^256 and not canonical
    len  len_plus_one, and len_minus_one where the count is positive (u64: the same two)
A substitute whose bytes equal the original changes nothing and is skipped; corpora count those skips."""
import re

L_ORDER = 2 ** 252 + 27742317777372353535851937790883648493
IDENTITY = bytes(32)
UNDECODABLE = bytes([1] + [0] * 31)
SUBSTITUTES = {"pt": ("identity", "other_point", "undecodable"), "fr": ("plus_one", "zero", "plus_l"), "len": ("len_plus_one", "len_minus_one"),
               "u64": ("len_plus_one", "len_minus_one")}
ONE_PER_FIELD = {"pt": "other_point", "fr": "plus_one", "len": "len_plus_one", "u64": "len_plus_one"}
ROW_VECTORS = ("comm_vars", "comm_derefs", "comm_ops", "comm_mem")               # the vectors of row commitments a RowSum runs over
MALFORMED, DECOMPRESS, VERIFY_INTERNAL, INVALID_NUM_INPUTS = -12, -11, -10, -3


# ------------------------------------------------------------------------------------------------ the walk
class _Walk:
    def __init__(self, blob):
        self.b, self.pos, self.fields = blob, 0, []

    def _take(self, name, kind, size):
        if self.pos + size > len(self.b):
            raise ValueError("%s at offset %d runs past the end (%d bytes)" % (name, self.pos, len(self.b)))
        self.fields.append((name, self.pos, kind))
        self.pos += size

    def u64(self, name, kind="len"):
        self._take(name, kind, 8)
        return int.from_bytes(self.b[self.pos - 8:self.pos], "little")

    def pt(self, name):
        self._take(name, "pt", 32)

    def fr(self, name):
        self._take(name, "fr", 32)

    def _vec(self, name, one):
        n = self.u64(name + ".len")
        if n > len(self.b):
            raise ValueError("%s.len = %d in a blob of %d bytes" % (name, n, len(self.b)))
        for i in range(n):
            one("%s[%d]" % (name, i))
        return n

    def pts(self, name):
        return self._vec(name, self.pt)

    def frs(self, name):
        return self._vec(name, self.fr)

    def sumcheck(self, name):                                   # ZKSumcheckProof: comm_polys, comm_evals, proofs of DotProductProof
        self.pts(name + ".comm_polys"); self.pts(name + ".comm_evals")

        def proof(p):
            self.pt(p + ".delta"); self.pt(p + ".beta"); self.frs(p + ".z"); self.fr(p + ".z_delta"); self.fr(p + ".z_beta")
        self._vec(name + ".proofs", proof)

    def dplog(self, name):                                      # DotProductProofLog
        self.pts(name + ".L"); self.pts(name + ".R"); self.pt(name + ".delta"); self.pt(name + ".beta"); self.fr(name + ".z1"); self.fr(name + ".z2")

    def r1cs(self):                                             # R1CSProof: NizkProof without rx, ry
        self.pts("comm_vars"); self.sumcheck("sc1")
        for i in range(4):
            self.pt("claims_phase2[%d]" % i)
        self.pt("pok.alpha"); self.fr("pok.z1"); self.fr("pok.z2")
        self.pt("prod.alpha"); self.pt("prod.beta"); self.pt("prod.delta")
        for i in range(5):
            self.fr("prod.z[%d]" % i)
        self.pt("eq1.alpha"); self.fr("eq1.z")
        self.sumcheck("sc2")
        self.pt("comm_vars_at_ry")
        self.dplog("polyeval")
        self.pt("eq2.alpha"); self.fr("eq2.z")

    def evals4(self, name):
        self.fr(name + ".init"); self.frs(name + ".read"); self.frs(name + ".write"); self.fr(name + ".audit")

    def batch(self, name):                                      # ProductCircuitEvalProofBatched: per layer its rounds' three coefficients, left, right
        def layer(p):
            self._vec(p + ".coeffs", self.frs)
            self.frs(p + ".left"); self.frs(p + ".right")
        self._vec(name + ".layers", layer)
        self.frs(name + ".dotp_left"); self.frs(name + ".dotp_right"); self.frs(name + ".dotp_weight")

    def done(self):
        if self.pos != len(self.b):
            raise ValueError("the walk ended at %d of %d bytes" % (self.pos, len(self.b)))
        return self.fields


def nizk(blob):
    w = _Walk(blob)
    w.r1cs(); w.frs("rx"); w.frs("ry")
    return w.done()


def snark(blob):
    w = _Walk(blob)
    w.r1cs()
    for k in range(3):
        w.fr("inst_evals[%d]" % k)
    w.pts("comm_derefs")
    w.evals4("eval_row"); w.evals4("eval_col"); w.frs("dotp_left"); w.frs("dotp_right")
    w.batch("proof_mem"); w.batch("proof_ops")
    w.frs("h_row_addr"); w.frs("h_row_read_ts"); w.fr("h_row_audit")
    w.frs("h_col_addr"); w.frs("h_col_read_ts"); w.fr("h_col_audit")
    w.frs("h_val"); w.frs("h_deref_row"); w.frs("h_deref_col")
    w.dplog("pe_ops"); w.dplog("pe_mem"); w.dplog("pe_derefs")
    return w.done()


def commitment(blob):
    w = _Walk(blob)
    for name in ("num_cons", "num_vars", "num_inputs", "batch_size", "num_ops", "num_mem_cells"):
        w.u64(name, "u64")
    w.pts("comm_ops"); w.pts("comm_mem")
    return w.done()


def value(blob, fields, name):
    """the integer a len / u64 field holds"""
    for n, off, kind in fields:
        if n == name:
            assert kind in ("len", "u64"), (name, kind)
            return int.from_bytes(blob[off:off + 8], "little")
    raise KeyError(name)


def group(name):
    """the struct member a field belongs to: its name without the indices (sc1.proofs[3].z[2] -> sc1.proofs[].z[])"""
    return re.sub(r"\[\d+\]", "[]", name)


def _indices(name):
    return tuple(int(x) for x in re.findall(r"\[(\d+)\]", name))


# ------------------------------------------------------------------------------------------------ substitutes
def substitute(blob, fields, field, what):
    """the blob with `field` = (name, offset, kind) replaced by its substitute `what`; None where that changes no byte, or where a count of 0 has
    no count - 1 (callers tell the two apart by kind)"""
    name, off, kind = field
    assert what in SUBSTITUTES[kind], (name, kind, what)
    if kind in ("len", "u64"):
        v = int.from_bytes(blob[off:off + 8], "little") + (1 if what == "len_plus_one" else -1)
        return None if v < 0 else blob[:off] + v.to_bytes(8, "little") + blob[off + 8:]
    cur = blob[off:off + 32]
    if kind == "pt":
        if what == "identity":
            new = IDENTITY
        elif what == "undecodable":
            new = UNDECODABLE
        else:
            pts = [o for _, o, k in fields if k == "pt"]
            at = pts.index(off)
            new = next(blob[o:o + 32] for o in pts[at + 1:] + pts[:at] if blob[o:o + 32] not in (cur, IDENTITY))
    else:
        raw = int.from_bytes(cur, "little")
        new = {"plus_one": (raw + 1) % L_ORDER, "zero": 0, "plus_l": raw + L_ORDER}[what].to_bytes(32, "little")
    return None if new == cur else blob[:off] + new + blob[off + 32:]


class Corpus:
    """mutants: [(field name, substitute name, bytes)]; skipped: [(field name, substitute name)] whose bytes would have equalled the original"""

    def __init__(self, blob, fields, picks):
        self.mutants, self.skipped = [], []
        for field, what in picks:
            m = substitute(blob, fields, field, what)
            if m is not None:
                self.mutants.append((field[0], what, m))
            elif field[2] in ("pt", "fr"):
                self.skipped.append((field[0], what))

    def __len__(self):
        return len(self.mutants)

    def check_skips(self, percent=1):
        """A substitute is skipped only where it equals the original — the identity in place of the identity, zero in place of zero — and at most
        1 % of a full or one-per-field corpus may be.  steering is exempt from the percentage (percent=None): it asks for the LAST row commitment
        with all three substitutes, and the last rows of a computation commitment are padding, commitments to zero rows: the identity itself."""
        assert all(what in ("identity", "zero") for _, what in self.skipped), self.skipped
        if percent is not None:
            assert 100 * len(self.skipped) <= percent * (len(self.mutants) + len(self.skipped)), self.skipped
        return len(self.skipped)


def full(blob, fields):
    """every substitute of every field"""
    return Corpus(blob, fields, [(f, what) for f in fields for what in SUBSTITUTES[f[2]]])


def one_per_field(blob, fields):
    """one mutant for every field: other_point for points, plus_one for scalars, count + 1 for counts"""
    return Corpus(blob, fields, [(f, ONE_PER_FIELD[f[2]]) for f in fields])


def _ends(fields):
    """of the fields of one group, those at the first and the last element of every vector of structs (or of vectors) on their path, and at the first
    element of the innermost vector"""
    keep = list(fields)
    depth = len(_indices(keep[0][0])) if keep else 0
    innermost = depth - 1 if keep and keep[0][0].endswith("]") else depth            # a member of a struct (x[3].len) has no innermost vector
    for d in range(depth):
        by_prefix = {}
        for f in keep:
            idx = _indices(f[0])
            by_prefix.setdefault(idx[:d], set()).add(idx[d])
        ok = {p: ({min(s)} if d == innermost else {min(s), max(s)}) for p, s in by_prefix.items()}
        keep = [f for f in keep if _indices(f[0])[d] in ok[_indices(f[0])[:d]]]
    return keep


def steering(blob, fields):
    """a pruned corpus for large sizes: of each vector of row commitments the first, second, middle and last point with all three point substitutes;
    every element of rx and ry with plus_one; and one one_per_field mutant from each remaining group of fields (a struct member; of a vector of structs
    the first and the last element)"""
    picks, groups = [], {}
    rows = {v: [f for f in fields if group(f[0]) == v + "[]"] for v in ROW_VECTORS}
    for v, fs in rows.items():
        for i in sorted({0, 1, len(fs) // 2, len(fs) - 1} & set(range(len(fs)))):
            picks += [(fs[i], what) for what in SUBSTITUTES["pt"]]
    for f in fields:
        g = group(f[0])
        if g in ("rx[]", "ry[]"):
            picks.append((f, "plus_one"))
        elif g[:-2] not in ROW_VECTORS:
            groups.setdefault(g, []).append(f)
    for fs in groups.values():
        picks += [(f, ONE_PER_FIELD[f[2]]) for f in _ends(fs)]
    return Corpus(blob, fields, picks)


# ------------------------------------------------------------------------------------------------ balanced counts
# Changing ONE count breaks the framing: every later field is read from the wrong place and the parser refuses the bytes.  A verifier also requires
# certain vectors to agree in length, and that is only reached by bytes that are well framed: here one vector loses its last element and another of
# the same set gains one (a copy of its own last element; 32 zero bytes, a valid point and a valid scalar, where it was empty), each with its count.
def agreeing_vectors(fields):
    """the sets of counted vectors a verifier requires to be equally long, by name: a sum-check's comm_polys / comm_evals / proofs, the L / R of
    every log dot-product proof, each product-circuit layer's left / right, a batched proof's dotp_left / dotp_right / dotp_weight"""
    lens = {name[:-4] for name, _, kind in fields if kind == "len"}
    sets = [[sc + ".comm_polys", sc + ".comm_evals", sc + ".proofs"] for sc in ("sc1", "sc2")]
    sets += [[d + ".L", d + ".R"] for d in ("polyeval", "pe_ops", "pe_mem", "pe_derefs") if d + ".L" in lens]
    for b in ("proof_mem", "proof_ops"):
        layers = sorted(n for n in lens if re.fullmatch(re.escape(b) + r"\.layers\[\d+\]\.left", n))
        sets += [[n, n[:-4] + "right"] for n in sorted(layers, key=_indices)]
        if b + ".dotp_left" in lens:
            sets.append([b + ".dotp_left", b + ".dotp_right", b + ".dotp_weight"])
    assert all(v in lens for s in sets for v in s), sets
    return sets


def _resize(blob, fields, vec, delta):
    """the edits [(offset, bytes removed, bytes put there)] that give vector `vec` one element more (delta = 1) or take its last (delta = -1)"""
    count_at = next(off for name, off, _ in fields if name == vec + ".len")
    n = int.from_bytes(blob[count_at:count_at + 8], "little")
    assert n + delta >= 0, vec
    spans = [(off, off + (8 if kind in ("len", "u64") else 32)) for name, off, kind in fields if name.startswith(vec + "[%d]" % (n - 1))] if n else []
    start, end = (min(s for s, _ in spans), max(e for _, e in spans)) if n else (count_at + 8, count_at + 8)
    body = (end, 0, blob[start:end] if n else IDENTITY) if delta > 0 else (start, end - start, b"")
    return [(count_at, 8, (n + delta).to_bytes(8, "little")), body]


def balanced(blob, fields):
    """[(name, bytes)], name "a -> b": within every set of agreeing_vectors, vector a shorter by one and the next of its set (the first again behind
    the last) longer by one, nothing else changed; a move out of an empty vector does not exist and is left out"""
    out = []
    for vecs in agreeing_vectors(fields):
        for k, a in enumerate(vecs):
            b = vecs[(k + 1) % len(vecs)]
            if value(blob, fields, a + ".len") == 0:
                continue
            m = blob
            for off, cut, put in sorted(_resize(blob, fields, a, -1) + _resize(blob, fields, b, 1), reverse=True):
                m = m[:off] + put + m[off + cut:]
            out.append(("%s -> %s" % (a, b), m))
    return out


# ------------------------------------------------------------------------------------------------ the verdict rule
def verdict_error(what, oracle_code, product_code):
    """None where the two verifiers' codes for a mutant made with substitute `what` are what they must be, else what is wrong.  Both reject; a
    non-canonical scalar and a changed count are MALFORMED to both; a decodable point and a canonical scalar get the same code from both; an
    undecodable point is DECOMPRESS or VERIFY_INTERNAL to the product (which decompresses row commitments early and defers group equations, where
    the oracle's sequential order can meet a failed equation first), and DECOMPRESS wherever the oracle says so."""
    o, p = oracle_code, product_code
    if o == 0 or p == 0:
        return "ACCEPTED (oracle %d, product %d)" % (o, p)
    if what in ("plus_l", "len_plus_one", "len_minus_one"):
        return None if o == p == MALFORMED else "want MALFORMED from both (oracle %d, product %d)" % (o, p)
    if what == "undecodable":
        if p not in (DECOMPRESS, VERIFY_INTERNAL) or (o == DECOMPRESS and p != DECOMPRESS):
            return "undecodable point: oracle %d, product %d" % (o, p)
        return None
    return None if o == p else "codes differ (oracle %d, product %d)" % (o, p)


def failures(corpus, oracle_codes, product_codes):
    """the mutants that break the verdict rule, each named by field and substitute"""
    assert len(corpus.mutants) == len(oracle_codes) == len(product_codes)
    out = []
    for (name, what, _), o, p in zip(corpus.mutants, oracle_codes, product_codes):
        err = verdict_error(what, o, p)
        if err:
            out.append("%s / %s: %s" % (name, what, err))
    return out


def differences(corpus, want, got):
    """where two lists of codes for the same corpus differ, each named by field and substitute"""
    assert len(corpus.mutants) == len(want) == len(got)
    return ["%s / %s: %d != %d" % (name, what, w, g) for (name, what, _), w, g in zip(corpus.mutants, want, got) if w != g]
