"""Operands and the plain big-integer reference for the device's arithmetic over GF(2^255-19) (field.h Fp, fp9.h F9, fp10.h F10, the point formulas
built on them, RFC 9496 encode / decode).  Needs no GPU and nothing of the product.

What is restated here and why:
    * arithmetic mod p, affine twisted Edwards addition (a = -1), ristretto255 Encode / Decode (RFC 9496 4.3.1, 4.3.2): THE reference;
    * the addition formulas (add-2008-hwcd-3, mixed and full) as polynomial maps on arbitrary field elements: what p9_madd, p10_madd, p10_add and the
      quad forms must return coordinate by coordinate, whether or not the operands are points;
    * the limb forms' unpack / add / sub / carry / product on Python integers, limb for limb as the headers' C bodies compute them: ONLY to know the
      limbs an operand of a product has, so that a host test can hold every case against the precondition its header states.  The expected VALUE of a
      device result never comes from these.
A 256-bit value is any integer below 2^256: the unpackers take every one ("loosely reduced")."""
import itertools
import random

P = 2 ** 255 - 19
L = 2 ** 252 + 27742317777372353535851937790883648493
D = (-121665 * pow(121666, -1, P)) % P
D2 = 2 * D % P
SQRT_M1 = pow(2, (P - 1) // 4, P)
INVSQRT_A_MINUS_D = 54469307008909316920995813868745141605393597292927456921205312896311721017578
M256 = 2 ** 256 - 1


def inv(x):
    return pow(x % P, P - 2, P)


def is_neg(x):
    return (x % P) & 1


def fabs(x):
    x %= P
    return P - x if x & 1 else x


# ------------------------------------------------------------------------------------------------ the value pool
F10_SHIFT = (0, 26, 51, 77, 102, 128, 153, 179, 204, 230)
NAMED = {"0": 0, "1": 1, "2": 2, "19": 19, "p-1": P - 1, "p": P, "p+1": P + 1, "2^255-1": 2 ** 255 - 1, "2^255": 2 ** 255, "2^255+18": 2 ** 255 + 18,
         "2p": 2 * P, "2^256-1": M256, "(p-1)/2": (P - 1) // 2, "d": D, "2d": D2, "sqrt(-1)": SQRT_M1}


def _pool():
    vals = list(NAMED.values())
    for k in range(1, 9):
        vals += [2 ** (29 * k), 2 ** (29 * k) - 1]
    for s in F10_SHIFT[1:]:
        vals += [2 ** s, 2 ** s - 1]
    seen, out = set(), []
    for v in vals:
        if v not in seen:
            seen.add(v); out.append(v)
    assert all(0 <= v <= M256 for v in out)
    return tuple(out)


POOL = _pool()
EXTREMES = (M256, 2 ** 255 - 1, P - 1)                            # every limb of every form at (or next to) its maximum
BINARY = tuple(itertools.product(POOL, POOL))                    # all pairs, for the operations of two operands


def sample_tuples(width, count, key):
    """count tuples of pool values, seeded by `key`: all-equal tuples of the EXTREMES first, then draws in which every second tuple takes half of its
    entries from the EXTREMES (so the limb maxima meet each other far more often than a uniform draw over the pool would let them)"""
    rng = random.Random(repr(("curve_cases", key, width)))
    out = [(e,) * width for e in EXTREMES]
    while len(out) < count:
        t = [rng.choice(POOL) for _ in range(width)]
        if len(out) & 1:
            for i in range(width):
                if rng.getrandbits(1):
                    t[i] = rng.choice(EXTREMES)
        out.append(tuple(t))
    return tuple(out)


QUADS = sample_tuples(4, 1031, "quads")                          # (a, b, c, d) of the compound operations
MADD_TUPLES = sample_tuples(7, 1031, "madd")                     # (X, Y, Z, T, yplusx, yminusx, xy2d)
ADD_TUPLES = sample_tuples(8, 1031, "add")                       # (X1, Y1, Z1, T1, X2, Y2, Z2, T2)


# ------------------------------------------------------------------------------------------------ the field operations of otti_k_fp_op, mod p
FP_OPS = {
    "mul": lambda a, b, c, d: a * b, "sqr": lambda a, b, c, d: a * a, "add": lambda a, b, c, d: a + b, "sub": lambda a, b, c, d: a - b,
    "neg": lambda a, b, c, d: -a, "carry": lambda a, b, c, d: (a - b) + (c + d), "repack": lambda a, b, c, d: a,
    "mul_sub_add": lambda a, b, c, d: (a - b) * (c + d), "mul_3a_2b": lambda a, b, c, d: 3 * a * 2 * b,
    "mul_f_e": lambda a, b, c, d: (2 * a - b) * (c - d), "mul_carried_f_g": lambda a, b, c, d: (2 * a - b) * (2 * c + d),
    "pow22523": lambda a, b, c, d: pow(a % P, 2 ** 252 - 3, P),
}
FORM_OPS = {                                                     # fp9.h has no square and no power, and normalises 2a - b before it multiplies it
    "fp8": tuple(FP_OPS), "f10": tuple(FP_OPS),
    "f9": tuple(o for o in FP_OPS if o not in ("sqr", "pow22523", "mul_f_e")),
}
OP_ARITY = {"mul": 2, "sqr": 1, "add": 2, "sub": 2, "neg": 1, "carry": 4, "repack": 1, "mul_sub_add": 4, "mul_3a_2b": 2, "mul_f_e": 4,
            "mul_carried_f_g": 4, "pow22523": 1}


def op_cases(op):
    """the (a, b, c, d) tuples an operation runs on: the pool, all its pairs, or the sampled quadruples"""
    n = OP_ARITY[op]
    if n == 1:
        return tuple((a, 0, 0, 0) for a in POOL)
    if n == 2:
        return tuple((a, b, 0, 0) for a, b in BINARY)
    return QUADS


def fp_ref(op, t):
    return FP_OPS[op](*t) % P


# ------------------------------------------------------------------------------------------------ limb forms, as the headers compute them
class Form:
    """limbs of `bits[i]` bits at `shift[i]`; 2^255 = 19 folds the top carry into limb 0"""

    def __init__(self, name, bits):
        self.name, self.bits, self.n = name, tuple(bits), len(bits)
        self.shift = tuple(sum(bits[:i]) for i in range(self.n))
        assert sum(bits) == 255
        self.mask = tuple((1 << b) - 1 for b in bits)
        pl = [(P >> self.shift[i]) & self.mask[i] for i in range(self.n)]
        self.two_p = tuple(2 * x for x in pl)

    def value(self, l):
        return sum(int(x) << s for x, s in zip(l, self.shift))

    def unpack(self, v):
        assert 0 <= v <= M256
        l = [(v >> self.shift[i]) & self.mask[i] for i in range(self.n)]
        l[0] += 19 * (v >> 255)
        return l

    def add(self, a, b):
        return [x + y for x, y in zip(a, b)]

    def sub(self, a, b):
        r = [x + t - y for x, y, t in zip(a, b, self.two_p)]
        assert all(0 <= x < 2 ** 32 for x in r)
        return r

    def carry(self, a):
        r = list(a)
        assert all(0 <= x < 2 ** 32 for x in r)
        for i in range(self.n - 1):
            r[i + 1] += r[i] >> self.bits[i]; r[i] &= self.mask[i]
        c = r[-1] >> self.bits[-1]; r[-1] &= self.mask[-1]; r[0] += 19 * c
        c = r[0] >> self.bits[0]; r[0] &= self.mask[0]; r[1] += c
        return r


class Form9(Form):
    MUL_BOUND = 2 ** 63.9                                        # fp9.h: 9 * max f_i * max g_j below this, limb 8 of either operand below 2^26

    def __init__(self):
        super().__init__("f9", [29] * 8 + [23])

    def reduced(self, l):                                        # fp9.h "reduced"
        return all(l[i] < 2 ** 29 + (2 ** 18 if i < 2 else 0) for i in range(8)) and l[8] < 2 ** 23 + 2

    def mul_ok(self, f, g):
        return 9 * max(f) * max(g) < self.MUL_BOUND and f[8] < 2 ** 26 and g[8] < 2 ** 26 and max(f) < 2 ** 32 and max(g) < 2 ** 32

    def mul_load(self, f, g):
        return 9 * max(f) * max(g) / self.MUL_BOUND

    def mul(self, f, g):                                         # the C body of f9_mul
        m, h, acc = self.mask[0], [0] * 9, 0
        for k in range(9, 17):
            acc += sum(f[i] * g[k - i] for i in range(9) if 0 <= k - i < 9)
            assert acc < 2 ** 64
            h[k - 9] = acc & m; acc >>= 29
        h[8] = acc
        assert h[8] < 2 ** 32
        r, acc = [0] * 9, 0
        for k in range(9):
            acc += sum(f[i] * g[k - i] for i in range(9) if 0 <= k - i < 9) + h[k] * 1216
            assert acc < 2 ** 64
            if k < 8:
                r[k] = acc & m; acc >>= 29
        r[8] = acc & 0x7fffff
        t = (acc >> 23) * 19 + r[0]
        r[0] = t & m; r[1] += t >> 29
        return r


class Form10(Form):
    F_BOUND, G_BOUND, SQR_BOUND = 2 ** 28.1, 2 ** 27.7, 2 ** 27   # fp10.h: f10_mul(f, g) and f10_sqr(f)

    def __init__(self):
        super().__init__("f10", [26, 25] * 5)

    def reduced(self, l):                                        # fp10.h "reduced"
        return all(l[i] <= 2 ** (25 if i & 1 else 26) + 2 ** 17 for i in range(10))

    def mul_ok(self, f, g):
        return max(f) < self.F_BOUND and max(g) < self.G_BOUND

    def mul_load(self, f, g):
        """ten products 2 f_i * 19 g_j against 2^64, the way the header's two bounds are derived: their product is the budget"""
        return max(f) * max(g) / (self.F_BOUND * self.G_BOUND)

    def mul(self, f, g):                                         # f10_mul and f10_reduce_columns
        h = [0] * 10
        for k in range(10):
            for i in range(10):
                j = (k - i) % 10
                x = 2 * f[i] if (i & 1) and (j & 1) else f[i]
                y = 19 * g[j] if i + j >= 10 else g[j]
                assert x < 2 ** 32 and y < 2 ** 32
                h[k] += x * y
            assert h[k] < 2 ** 64
        r = [0] * 10
        for i in range(9):
            h[i + 1] += h[i] >> self.bits[i]; r[i] = h[i] & self.mask[i]
            assert h[i + 1] < 2 ** 64
        c = h[9] >> 25; r[9] = h[9] & self.mask[9]
        t = r[0] + 19 * c
        r[0] = t & self.mask[0]; t >>= 26
        t += r[1]; r[1] = t & self.mask[1]; t >>= 25
        r[2] += t
        return r


F9, F10 = Form9(), Form10()
FORMS = {"f9": F9, "f10": F10}


class Products:
    """the products a computation reaches: per name, the operand limbs' maxima of every case (precondition) and the largest load seen"""

    def __init__(self, form):
        self.form, self.load, self.bad, self.count, self.maxfg = form, {}, [], {}, {}

    def mul(self, name, f, g):
        if not self.form.mul_ok(f, g):
            self.bad.append((name, max(f), max(g)))
        self.load[name] = max(self.load.get(name, 0.0), self.form.mul_load(f, g))
        self.maxfg[name] = max(self.maxfg.get(name, 0), max(f) * max(g))
        self.count[name] = self.count.get(name, 0) + 1
        return self.form.mul(f, g)

    def sub(self, name, a, b):
        if not self.form.reduced(b):
            self.bad.append((name + ": subtrahend not reduced", max(a), max(b)))
        return self.form.sub(a, b)


class BoundForm:
    """a form on limb UPPER BOUNDS instead of limbs: what the headers' own reasoning gives for an operand, whatever the case.  Every unpacked, carried
    or multiplied value is "reduced" (the header's definition, limb by limb), a sum has the sum of the bounds, a - b + 2p the bound of a plus 2p."""

    def __init__(self, form):
        self.real, self.name, self.n, self.two_p = form, form.name, form.n, form.two_p
        if form.name == "f9":
            self.top = [2 ** 29 + 2 ** 18 - 1] * 2 + [2 ** 29 - 1] * 6 + [2 ** 23 + 1]
        else:
            self.top = [2 ** (25 if i & 1 else 26) + 2 ** 17 for i in range(10)]
        assert form.reduced(self.top)

    def unpack(self, v):
        return list(self.top)

    def add(self, a, b):
        return [x + y for x, y in zip(a, b)]

    def sub(self, a, b):
        return [x + t for x, t in zip(a, self.two_p)]

    def carry(self, a):
        assert all(x < 2 ** 32 for x in a)
        return list(self.top)

    def reduced(self, l):
        return all(x <= t for x, t in zip(l, self.top))

    def mul_ok(self, f, g):
        return self.real.mul_ok(f, g)

    def mul_load(self, f, g):
        return self.real.mul_load(f, g)

    def mul(self, f, g):
        return list(self.top)


def limbs_fp_op(rec, op, t):
    """the limb computation of one otti_k_fp_op case in rec.form, products and subtractions recorded; returns the result's limbs"""
    F = rec.form
    x, y, z, w = (F.unpack(v) for v in t)
    if op == "mul":
        return rec.mul(op, x, y)
    if op == "sqr":
        if F.name == "f10" and not max(x) < Form10.SQR_BOUND:
            rec.bad.append((op, max(x), max(x)))
        return rec.mul(op, x, x)
    if op == "add":
        return F.add(x, y)
    if op == "sub":
        return rec.sub(op, x, y)
    if op == "neg":
        return rec.sub(op, [0] * F.n, x)
    if op == "carry":
        return F.carry(F.add(rec.sub(op, x, y), F.add(z, w)))
    if op == "repack":
        return x
    if op == "mul_sub_add":
        return rec.mul(op, rec.sub(op, x, y), F.add(z, w))
    if op == "mul_3a_2b":
        return rec.mul(op, F.add(F.add(x, x), x), F.add(y, y))
    if op == "mul_f_e":
        return rec.mul(op, rec.sub(op, F.add(x, x), y), rec.sub(op, z, w))
    if op == "mul_carried_f_g":
        return rec.mul(op, F.carry(rec.sub(op, F.add(x, x), y)), F.add(F.add(z, z), w))
    raise KeyError(op)


def limbs_niels(rec, n3, neg):
    """n9_unpack / n10_unpack, then n9_negate / n10_negate: F9 leaves -xy2d uncarried, F10 carries it"""
    F = rec.form
    yp, ym, xy = (F.unpack(v) for v in n3)
    if neg:
        yp, ym = ym, yp
        xy = rec.sub("negate", [0] * F.n, xy)
        if F.name == "f10":
            xy = F.carry(xy)
    return yp, ym, xy


def limbs_madd(rec, p4, niels):
    """p9_madd / p10_madd on limbs; p4: four limb vectors (X, Y, Z, T), niels: three (yplusx, yminusx, xy2d)"""
    F = rec.form
    X, Y, Z, T = p4
    yp, ym, xy = niels
    a = rec.mul("A = (Y-X) yminusx", rec.sub("Y-X", Y, X), ym)
    b = rec.mul("B = (Y+X) yplusx", F.add(Y, X), yp)
    c = rec.mul("C = T xy2d", T, xy)
    d = F.add(Z, Z)
    e, f, g, h = rec.sub("E", b, a), rec.sub("F", d, c), F.add(d, c), F.add(b, a)
    if F.name == "f9":
        f = F.carry(f)
        return [rec.mul("X = E F", e, f), rec.mul("Y = G H", g, h), rec.mul("Z = F G", f, g), rec.mul("T = E H", e, h)]
    return [rec.mul("X = F E", f, e), rec.mul("Y = H G", h, g), rec.mul("Z = F G", f, g), rec.mul("T = H E", h, e)]


def limbs_add10(rec, p4, q4):
    """p10_add on limbs"""
    F = rec.form
    X1, Y1, Z1, T1 = p4
    X2, Y2, Z2, T2 = q4
    a = rec.mul("A = (Y1-X1)(Y2-X2)", rec.sub("Y1-X1", Y1, X1), rec.sub("Y2-X2", Y2, X2))
    b = rec.mul("B = (Y1+X1)(Y2+X2)", F.add(Y1, X1), F.add(Y2, X2))
    c = rec.mul("C = (T1 T2) 2d", rec.mul("T1 T2", T1, T2), F.unpack(D2))
    d = rec.mul("Z1 Z2", Z1, Z2); d = F.add(d, d)
    e, f, g, h = rec.sub("E", b, a), rec.sub("F", d, c), F.add(d, c), F.add(b, a)
    return [rec.mul("X = F E", f, e), rec.mul("Y = H G", h, g), rec.mul("Z = F G", f, g), rec.mul("T = H E", h, e)]


# ------------------------------------------------------------------------------------------------ the addition formulas as polynomial maps mod p
def madd_ref(p4, n3, neg=False):
    X, Y, Z, T = p4
    yp, ym, xy = n3
    if neg:
        yp, ym, xy = ym, yp, -xy
    a, b, c, d = (Y - X) * ym, (Y + X) * yp, T * xy, 2 * Z
    e, f, g, h = b - a, d - c, d + c, b + a
    return (e * f % P, g * h % P, f * g % P, e * h % P)


def add_ref(p4, q4):
    X1, Y1, Z1, T1 = p4
    X2, Y2, Z2, T2 = q4
    a, b, c, d = (Y1 - X1) * (Y2 - X2), (Y1 + X1) * (Y2 + X2), T1 * T2 * D2, 2 * Z1 * Z2
    e, f, g, h = b - a, d - c, d + c, b + a
    return (e * f % P, g * h % P, f * g % P, e * h % P)


# ------------------------------------------------------------------------------------------------ the group: affine points (x, y), -x^2 + y^2 = 1 + d x^2 y^2
O = (0, 1)
TORSION4 = (O, (0, P - 1), (SQRT_M1, 0), (P - SQRT_M1, 0))       # E[4]: encode(P + T) == encode(P) for each (the ristretto coset)


def on_curve(pt):
    x, y = pt
    return (-x * x + y * y - 1 - D * x * x * y * y) % P == 0


def aff_add(p, q):
    (x1, y1), (x2, y2) = p, q
    k = D * x1 * x2 * y1 * y2 % P
    return ((x1 * y2 + y1 * x2) * inv(1 + k) % P, (y1 * y2 + x1 * x2) * inv(1 - k) % P)


def aff_neg(p):
    return ((-p[0]) % P, p[1])


def aff_mul(k, p):
    r = O
    while k:
        if k & 1:
            r = aff_add(r, p)
        p = aff_add(p, p); k >>= 1
    return r


def extended(pt, scale=1, lift=False):
    """(X, Y, Z, T) of an affine point with every coordinate times `scale`; lift: the representative + p where it still fits 256 bits"""
    x, y = pt
    c = [x * scale % P, y * scale % P, scale % P, x * y * scale % P]
    if lift:
        c = [v + P if v + P <= M256 else v for v in c]
    return tuple(c)


def affine(p4):
    X, Y, Z, T = (v % P for v in p4)
    assert Z != 0 and (T * Z - X * Y) % P == 0
    zi = inv(Z)
    return (X * zi % P, Y * zi % P)


def niels(pt):
    x, y = pt
    return ((y + x) % P, (y - x) % P, D2 * x * y % P)


NIELS_IDENTITY = (1, 1, 0)


def sqrt_ratio_m1(u, v):
    u %= P; v %= P
    v3 = v * v * v % P; v7 = v3 * v3 * v % P
    r = u * v3 * pow(u * v7 % P, (P - 5) // 8, P) % P
    check = v * r * r % P
    correct, flipped, flipped_i = check == u, check == (-u) % P, check == (-u * SQRT_M1) % P
    if flipped or flipped_i:
        r = r * SQRT_M1 % P
    return (correct or flipped), fabs(r)


def rist_encode(p4):
    """RFC 9496 4.3.2 on extended coordinates (any projective scaling)"""
    X, Y, Z, T = (v % P for v in p4)
    u1, u2 = (Z + Y) * (Z - Y) % P, X * Y % P
    _, invsqrt = sqrt_ratio_m1(1, u1 * u2 * u2)
    den1, den2 = invsqrt * u1 % P, invsqrt * u2 % P
    zinv = den1 * den2 * T % P
    ix, iy = X * SQRT_M1 % P, Y * SQRT_M1 % P
    ench = den1 * INVSQRT_A_MINUS_D % P
    if is_neg(T * zinv):
        x, y, deninv = iy, ix, ench
    else:
        x, y, deninv = X, Y, den2
    if is_neg(x * zinv):
        y = -y
    return fabs(deninv * (Z - y)).to_bytes(32, "little")


DECODE_RULES = ("non-canonical s", "negative s", "non-square", "t < 0", "y = 0")


def rist_decode(b):
    """RFC 9496 4.3.1: (affine point, None), or (None, the rule that refuses the encoding) — the oracle's ristretto.c rejects in this order"""
    s = int.from_bytes(bytes(b), "little")
    if s >= P:
        return None, DECODE_RULES[0]
    if s & 1:
        return None, DECODE_RULES[1]
    ss = s * s % P
    u1, u2 = (1 - ss) % P, (1 + ss) % P
    u2s = u2 * u2 % P
    v = (-D * u1 * u1 - u2s) % P
    was_square, invsqrt = sqrt_ratio_m1(1, v * u2s)
    dx = invsqrt * u2 % P; dy = invsqrt * dx * v % P
    x = fabs(2 * s * dx); y = u1 * dy % P; t = x * y % P
    if not was_square:
        return None, DECODE_RULES[2]
    if is_neg(t):
        return None, DECODE_RULES[3]
    if y == 0:
        return None, DECODE_RULES[4]
    return (x, y), None


def refused_encodings():
    """one 32-byte input per rejection rule of Decode, the smallest that the rule (and no earlier one) refuses"""
    out = {DECODE_RULES[0]: P + 2, DECODE_RULES[1]: 1}           # p + 2 < 2^255 (bit 255 clear, even after reduction: 2): only the canonical test refuses it
    s = 2
    while len(out) < 4:
        _, why = rist_decode(s.to_bytes(32, "little"))
        if why in DECODE_RULES[2:4] and why not in out:
            out[why] = s
        s += 2
    out[DECODE_RULES[4]] = P - 1                                 # s = -1: u1 = 1 - s^2 = 0, so y = 0 (and t = 0 is not negative, and -16 is a square)
    res = {k: v.to_bytes(32, "little") for k, v in out.items()}
    for k, b in res.items():
        assert rist_decode(b) == (None, k), k
    return res


def words(v):
    return int(v).to_bytes(32, "little")
