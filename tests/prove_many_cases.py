"""What test_gpu_prove_many.py proves: per instance, SEVEN resident witnesses that between them reach every hand-over of a proof's witness-only work —
(1) the satisfying assignment, (2) the same keeping its rows, (3) keeping its products, (4) keeping both, (5) one variable scattered away
(unsatisfiable), (6) all-zero variables, (7) another handle whose inputs were replaced through set_inputs — with seeds bytes([k + 1]) * 32, and the
single proofs NIZK.prove makes of each, once, as the yardstick every prove_many call is held against byte for byte."""
import numpy as np

import otti_amd as oa

LABEL = b"many"
INVALID_NUM_VARS = -4                                      # OTTI_ERR_INVALID_NUM_VARS

INSTANCES = {"uniform-2^6": lambda: oa.synth_r1cs(1 << 6, 3, 2), "uniform-2^12": lambda: oa.synth_r1cs(1 << 12, 10, 1),
             "compiler-like-2^12": lambda: oa.synth_r1cs_compiler_like(1 << 12, 10, 5)}
# of the seven, those that keep no products are 1, 2, 5, 6, 7 and those that keep no rows 1, 3, 5, 6, 7: five each, one chunk.  The rows are summed
# jointly on every instance here; the products only where the by-row matrices have the row-per-quad layout (prove_many.cpp front_rule: the
# compiler-like instance), unless OTTI_PROVE_MANY_RULE=0 sets that rule aside
LACK_PRODUCTS = LACK_ROWS = 5
SATISFYING, UNSATISFIABLE = (0, 1, 2, 3), 4


def seed(k):
    return bytes([k + 1]) * 32


class Case:
    def __init__(self, name):
        r = INSTANCES[name]()
        self.name, self.r = name, r
        self.inst = oa.Instance.new(r["num_cons"], r["num_vars"], r["num_inputs"], r["A"], r["B"], r["C"])
        self.gens = oa.NIZKGens.new(r["num_cons"], r["num_vars"], r["num_inputs"])
        self.inputs = oa.InputsAssignment.new(r["inputs"])
        self.quad = name.startswith("compiler-like")
        vars_ = oa.VarsAssignment.new(r["vars"])
        new = lambda v=vars_: oa.Witness(self.inst, v, self.inputs)   # noqa: E731
        w = [new() for _ in range(5)]
        w[1].keep_rows(self.inst, self.gens)
        w[2].keep_products(self.inst)
        w[3].keep_rows(self.inst, self.gens)
        w[3].keep_products(self.inst)
        w[4].scatter(self.inst, np.array([5], dtype=np.int64), np.array([123456789], dtype=np.int64))
        w.append(new(oa.VarsAssignment.new(np.zeros_like(np.asarray(r["vars"])))))
        other = np.asarray(r["inputs"], dtype=np.uint8).copy()
        other[:, 0] ^= 1                                               # every input's lowest bit flipped: canonical still
        w.append(new())
        w[6].set_inputs(self.inst, other)
        self.wits = w
        self.item_inputs = [self.inputs] * 6 + [oa.InputsAssignment.new(other)]
        self.singles = [oa.NIZK.prove(self.inst, w[k], None, self.gens, LABEL, seed(k)).bytes for k in range(7)]

    def from_front(self, rule=True):
        """(products_from_front, rows_from_front) of a call over the seven with the default budget"""
        return (LACK_PRODUCTS if self.quad or not rule else 0, LACK_ROWS)

    def state(self):
        """everything a caller can see of the seven handles"""
        return [(w.info, w.rows_info(), w.products_info(), w.scatter_info()) for w in self.wits]

    def many(self, order=range(7), threads=0, seeds="own", details=True):
        order = list(order)
        sd = [seed(k) for k in order] if seeds == "own" else seeds
        return oa.NIZK.prove_many(self.inst, [self.wits[k] for k in order], self.gens, LABEL, seeds=sd, threads=threads, details=details)

    def assert_bytes(self, proofs, order=range(7)):
        for p, k in zip(proofs, order):
            assert p is not None and p.bytes == self.singles[k], (self.name, "witness", k + 1)
