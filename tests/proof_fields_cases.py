"""What the proof-field tests share beyond the field map (proof_fields.py): one instance held by both implementations — the CPU oracle and the
product — and the calls whose verdicts are compared on it: the oracle's verifier, the product's single verifier (the C entry's return code) and
the product's batched verifier.  Used by test_proof_fields_host.py (oracle proofs, no GPU) and test_gpu_proof_fields.py (the product's proofs,
device routes)."""
import concurrent.futures
import time

import numpy as np

import otti_amd as oa
import orc
import proof_fields as pf
import snark_verify_many_cases as sm
import verify_many_cases as vm

LABEL = b"fields"
SEED = bytes([0x5e]) * 32


class NizkCase:
    def __init__(self, r):
        self.r, self.inputs = r, r["inputs"]
        dims = (r["num_cons"], r["num_vars"], r["num_inputs"])
        self.oi, self.og = orc.OInstance(*dims, r["A"], r["B"], r["C"]), orc.OGens(*dims)
        self.inst, self.gens = oa.Instance.new(*dims, r["A"], r["B"], r["C"]), oa.NIZKGens.new(*dims)
        self.N, self.V = self.oi.num_cons, self.oi.num_vars                                # padded
        assert self.inst.dims[:2] == (self.N, self.V)

    def oracle_proof(self):
        return orc.nizk_prove(self.oi, self.r["vars"], self.inputs, self.og, LABEL, SEED)[0]

    def device_proof(self):
        wit = oa.Witness(self.inst, oa.VarsAssignment.new(self.r["vars"]), oa.InputsAssignment.new(self.inputs))
        return oa.NIZK.prove(self.inst, wit, None, self.gens, LABEL, SEED).bytes

    fields = staticmethod(pf.nizk)

    def oracle(self, blob, inputs=None):
        return int(orc.nizk_verify(self.oi, self.inputs if inputs is None else inputs, self.og, blob, LABEL))

    def product(self, blob, inputs=None):
        return vm.single_code(self.inst, self.gens, LABEL, blob, self.inputs if inputs is None else inputs)

    def product_many(self, blobs, threads=0):
        return vm.many(self.inst, self.gens, LABEL, [(b, self.inputs) for b in blobs], threads)


class SnarkCase:
    def __init__(self, r):
        self.r, self.inputs = r, r["inputs"]
        dims = (r["num_cons"], r["num_vars"], r["num_inputs"])
        self.nz = int(max(r["A"].size, r["B"].size, r["C"].size))
        self.oi, self.og = orc.OInstance(*dims, r["A"], r["B"], r["C"]), orc.OSnarkGens(*dims, self.nz)
        self.oc = orc.OSnarkComm.encode(self.oi, self.og)                                  # the oracle's prover copy
        self.comm_bytes = self.oc.bytes
        self.ov = orc.OSnarkComm.parse(self.comm_bytes)                                    # both verifiers hold the commitment only
        self.gens = oa.SNARKGens.new(*dims, self.nz)
        self.comm = oa.ComputationCommitment.from_bytes(self.comm_bytes)
        self.N, self.V = self.oi.num_cons, self.oi.num_vars

    def oracle_proof(self, seed=SEED):
        return orc.snark_prove(self.oi, self.oc, self.r["vars"], self.inputs, self.og, LABEL, seed)[0]

    def device_proofs(self, seeds=(SEED,)):
        """the product's own commitment (asserted equal to the oracle's) and its proofs from it, one per seed"""
        r = self.r
        inst = oa.Instance.new(r["num_cons"], r["num_vars"], r["num_inputs"], r["A"], r["B"], r["C"])
        prover_comm = oa.ComputationCommitment.encode(inst, self.gens)
        assert prover_comm.bytes == self.comm_bytes, "the product's computation commitment differs from the oracle's"
        wit = oa.Witness(inst, oa.VarsAssignment.new(r["vars"]), oa.InputsAssignment.new(self.inputs))
        return [oa.SNARK.prove(inst, prover_comm, wit, None, self.gens, LABEL, seed).bytes for seed in seeds]

    fields = staticmethod(pf.snark)

    def oracle(self, blob, inputs=None, comm=None):
        return int(orc.snark_verify(comm or self.ov, self.inputs if inputs is None else inputs, self.og, blob, LABEL))

    def product(self, blob, inputs=None, comm=None):
        return sm.single_code(comm or self.comm, self.gens, LABEL, blob, self.inputs if inputs is None else inputs)

    def product_many(self, blobs, threads=0, comm=None):
        return sm.many(comm or self.comm, self.gens, LABEL, [(b, self.inputs) for b in blobs], threads)

    def parse_both(self, comm_bytes):
        """(oracle commitment, product commitment) re-parsed from bytes, None where that side refuses them"""
        try:
            o = orc.OSnarkComm.parse(comm_bytes)
        except ValueError:
            o = None
        try:
            p = oa.ComputationCommitment.from_bytes(comm_bytes)
        except oa.SpartanError:
            p = None
        return o, p


ORACLE_THREADS = 8


def codes(verify, corpus, threads=1):
    """verify's code for every mutant, in order.  threads > 1 is for the oracle only: its verifier is plain re-entrant C (no state outside its
    arguments), ctypes releases the interpreter lock around it, and a corpus's cost is mostly the oracle's; the product is asked one call at a time"""
    blobs = [m for _, _, m in corpus.mutants]
    if threads <= 1:
        return [verify(b) for b in blobs]
    with concurrent.futures.ThreadPoolExecutor(threads) as pool:
        return list(pool.map(verify, blobs))


class Run:
    """a corpus with the oracle's and the single product verifier's code for every mutant, taken once"""

    def __init__(self, case, proof, corpus, what, skip_percent=1):
        self.case, self.proof, self.corpus = case, proof, corpus
        skipped = corpus.check_skips(skip_percent)
        assert case.oracle(proof) == 0 and case.product(proof) == 0, "the unchanged proof must be accepted by both"
        t0 = time.time()
        self.oracle = codes(case.oracle, corpus, ORACLE_THREADS)
        t1 = time.time()
        self.product = codes(case.product, corpus)
        t2 = time.time()
        undec = sum(1 for (_, w, _), o, p in zip(corpus.mutants, self.oracle, self.product) if w == "undecodable" and o != p)
        print("%s: %d mutants, %d skipped (equal to the original), oracle %.1f s, product %.1f s; undecodable points where the codes differ: %d"
              % (what, len(corpus), skipped, t1 - t0, t2 - t1, undec))

    def failures(self):
        return pf.failures(self.corpus, self.oracle, self.product)

    def with_good(self, order=None):
        """(blobs, expected single codes): the corpus in `order` with the unchanged proof at both ends and in the middle"""
        order = list(range(len(self.corpus))) if order is None else order
        blobs = [self.corpus.mutants[i][2] for i in order]; want = [self.product[i] for i in order]
        mid = len(order) // 2
        return [self.proof] + blobs[:mid] + [self.proof] + blobs[mid:] + [self.proof], [0] + want[:mid] + [0] + want[mid:] + [0]

    def many_differences(self, got, order=None):
        """got: the batched verifier's codes for with_good(order)'s blobs; the differences from the single codes, named"""
        order = list(range(len(self.corpus))) if order is None else order
        _, want = self.with_good(order)
        assert len(got) == len(want)
        mid = len(order) // 2
        names = ["good"] + ["%s / %s" % self.corpus.mutants[i][:2] for i in order[:mid]] + ["good"] + ["%s / %s" % self.corpus.mutants[i][:2] for i in order[mid:]] + ["good"]
        return ["%s: single %d, batched %d" % (n, w, g) for n, w, g in zip(names, want, got) if w != g]


def interleaved(n, ways=4):
    """0 .. n - 1 ordered so that every run of `ways` consecutive items comes from `ways` different stretches of the wire form"""
    q = -(-n // ways)
    return [j * q + k for k in range(q) for j in range(ways) if j * q + k < n]


def inputs_plus_one(inputs32, k):
    """the inputs (canonical bytes) with element k replaced by (x + 1) mod l"""
    out = np.array(inputs32, dtype=np.uint8, copy=True)
    x = (int.from_bytes(out[k].tobytes(), "little") + 1) % pf.L_ORDER
    out[k] = np.frombuffer(x.to_bytes(32, "little"), dtype=np.uint8)
    return out
