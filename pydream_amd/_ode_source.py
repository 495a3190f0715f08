"""The C++ text pydream_amd.likelihoods.MassActionODELogLike generates for csrc/dz_ode.h and csrc/dz_ode_group.h: one description of the
checked network (_Network) and the three emitters that read it -- one lane with every sum whole, one lane reaction by reaction, and the
lane group.  The text is the interface to both builds and the key of the kernel cache: it does not change with the code that writes it."""
import numpy as np

from ._ode_values import _INT, Monomial, RateLaw

_LOG_2PI_HALF = 0.5 * np.log(2.0 * np.pi)


def _hexlit(v):
    """A C++17 hexadecimal floating literal: the double exactly."""
    v = float(v)
    return "(%s)" % v.hex() if np.isfinite(v) else ("(__builtin_huge_val())" if v > 0 else "(-__builtin_huge_val())")


def _rate(rate):
    """A reaction's rate constant: the third element itself, or a RateLaw's rate."""
    return rate.rate if isinstance(rate, RateLaw) else rate


def _orders(reaction):
    """A reaction's kinetic orders {species: order}: the reactants' coefficients unless a RateLaw's order replaces them."""
    law = reaction[2]
    return dict(law.order) if isinstance(law, RateLaw) and law.order is not None else reaction[0]


def _factors(reaction):
    return reaction[2].factors if isinstance(reaction[2], RateLaw) else ()


def _kinetic_species(reaction):
    """The species a reaction's rate depends on, ascending: those with a kinetic order and those of its Hill factors."""
    return sorted(set(_orders(reaction)) | {f.species for f in _factors(reaction)})


def _hill_slots(reactions):
    """The distinct (K, n) pairs of the network's Hill factors, in the order of their first use: one slot each (csrc/dz_ode.h).
    A mapping from (type(K), K, n) -- the index 1 and the constant 1.0 are two -- to the slot's number."""
    slots = {}
    for rx in reactions:
        for f in _factors(rx):
            slots.setdefault((type(f.K), f.K, f.n), len(slots))
    return slots


def _indices_read(constants):
    """The parameter indices the constants read, bare or inside a monomial, ascending: those whose x is tested for finiteness."""
    return sorted({c for c in constants if isinstance(c, _INT)} | {i for c in constants if isinstance(c, Monomial) for i in c.indices})


def _rate_indices(reactions):
    return _indices_read([_rate(r) for _, _, r in reactions])


def _slot_indices(slots):
    return _indices_read([K for _, K, _ in slots])


def _dexp10(arg):
    return "dzode::dexp(%s * 2.302585092994046)" % arg


def _mono_value(m):
    """The C++ expression of a monomial's value: the sum in ascending index, an exponent of +-1 as a plain add or subtract."""
    out = _hexlit(m.log10_factor)
    for i, e in m.exponents:
        out += " + x[%d]" % i if e == 1.0 else " - x[%d]" % i if e == -1.0 else " + %s * x[%d]" % (_hexlit(e), i)
    return _dexp10("(%s)" % out)


def _finite(indices, values=()):
    """The liveness tests of the coordinates x[i] and of the named values."""
    return ["dzode::finite(x[%d])" % i for i in indices] + ["dzode::finite(%s)" % v for v in values]


class _Network:
    """What the emitters read, made once per source() from the checked MassActionODELogLike: S, the reactions, the observables and
    log10; the stoichiometry N, the rate constants (`rates`: a RateLaw's own) and the kinetic species per reaction; the Hill slots
    (_hill_slots); mono (MassActionODELogLike._monomials), the largest event count, the equilibrate flag; items (the entry points for
    several conditions per point) and lanes."""

    def __init__(self, like):
        self.S, self.reactions, self.observables, self.log10 = like.n_species, like.reactions, like.observables, like.log10
        self.mono, self.events, self.equilibrate = like._monomials(), like._max_events(), like._equilibrates()
        self.items, self.lanes, self.noise = like.conditions is not None, like.lanes_per_point, like.noise
        self.settle = like._settles()          # the last output time is +inf (csrc/dz_ode.h, STEADY OUTPUT)
        self.inputs = [(u.species, u.gain) for u in like.inputs or ()]      # (species, gain): the tables are the data block's
        self.view = like._view_size() if like._has_view() else 0            # P of a network whose conditions view the point (csrc/dz_ode.h, VIEWS)
        self.normalize = like.normalize        # None, or O entries None | Normalize (csrc/dz_ode.h, NORMALISED READOUTS)
        self.knots = like._max_input_knots() if self.normalize else 0       # Kmax: the norm records sit behind the knots' records
        self.R = len(self.reactions)
        self.N = np.zeros((self.S, self.R), dtype=np.int64)
        for r, (reac, prod, _) in enumerate(self.reactions):
            for s, c in reac.items():
                self.N[s, r] -= c
            for s, c in prod.items():
                self.N[s, r] += c
        self.rates = [_rate(rate) for _, _, rate in self.reactions]
        self.kinetic = [_kinetic_species(reaction) for reaction in self.reactions]
        self.slots = _hill_slots(self.reactions)

    def constant(self, c):
        """(the C++ expression of a rate constant or a slot's K, the parameter indices it reads): a Monomial, a sampled constant under
        the rate scale, or a literal"""
        if isinstance(c, Monomial):
            return _mono_value(c), c.indices
        if isinstance(c, _INT):
            return _dexp10("x[%d]" % c) if self.log10 else "x[%d]" % c, (c,)
        return _hexlit(c), ()

    def input_of(self, s):
        """the number of the input that species s carries, or None"""
        return next((i for i, (species, _) in enumerate(self.inputs) if species == s), None)

    def slot_of(self, f):
        return self.slots[type(f.K), f.K, f.n]

    def rate_code(self, kname, first):
        """(v(r), dv(r, q)): the expressions of reaction r's rate and of its derivative by y_q under an emitter's names -- kname[r] for
        the rate constant, k[first + m] (the lane group: k[z + first + m]) for slot m."""
        slotname = "k[%d]" if self.lanes == 1 else "k[z + %d]"
        kn = lambda f: slotname % (first + self.slot_of(f))      # noqa: E731

        def v(r):
            """v = k * prod y^order (ascending species) * prod h_m (in the order given), left to right."""
            reaction = self.reactions[r]
            return _product([kname[r]] + _rate_factors(_orders(reaction)) + [_hill_value(f, kn(f)) for f in _factors(reaction)])

        def dv(r, q):
            """dv / dy_q: the product rule's sum in the order of the product -- the mass-action term (q has a kinetic order), then one term per
            Hill factor on q, each the product v with that one factor replaced by its derivative.  A reaction without factors: the one product
            it always was."""
            reaction = self.reactions[r]
            order, hills = _orders(reaction), _factors(reaction)
            values = [_hill_value(f, kn(f)) for f in hills]
            terms = []
            if q in order:
                c = order[q]
                terms.append(_product([kname[r]] + (["%d.0" % c] if c > 1 else []) + _rate_factors(order, skip=q) + values))
            for m, f in enumerate(hills):
                if f.species == q:
                    terms.append(_product([kname[r]] + _rate_factors(order) + values[:m] + [_hill_slope(f, kn(f))] + values[m + 1:]))
            return terms[0] if len(terms) == 1 else " + ".join("(%s)" % t for t in terms)
        return v, dv


def _hill_value(f, kn):
    """A Hill factor at y: yn the repeated product of y, den = Kn + yn, yn / den (activation) or Kn / den (repression).  kn: Kn's name."""
    yn = " * ".join(["y[%d]" % f.species] * f.n)
    return "((%s) / (%s + %s))" % (yn if f.kind == "activation" else kn, kn, yn)


def _hill_slope(f, kn):
    """Its derivative: num = ((n * Kn) * y) * y ... (n - 1 factors of y, left to right; n = 1: Kn itself), den = Kn + yn,
    +-num / (den * den): the sign is applied to the quotient."""
    yn = " * ".join(["y[%d]" % f.species] * f.n)
    num = " * ".join((["%d.0" % f.n] if f.n > 1 else []) + [kn] + ["y[%d]" % f.species] * (f.n - 1))
    return "(%s(%s) / ((%s + %s) * (%s + %s)))" % ("" if f.kind == "activation" else "-", num, kn, yn, kn, yn)


def _slot_lines(net, first):
    """The one-lane rates()' statements for the Hill slots, k[first + m] = Kn, and their liveness tests (csrc/dz_ode.h, RATE LAWS)."""
    L, tests = [], _finite(_slot_indices(net.slots))
    for (_, K, n), m in net.slots.items():
        L.append("        const double K%d = %s;" % (m, net.constant(K)[0]))
        L.append("        k[%d] = %s;" % (first + m, " * ".join(["K%d" % m] * n)))
        tests += _finite((), ["K%d" % m, "k[%d]" % (first + m)]) + ["k[%d] > 0.0" % (first + m)]
    return L, tests


def _input_lines(net, first):
    """The one-lane rates()' statements for the inputs' gains, k[first + i] = g_i (1 without a gain), and their liveness tests
    (csrc/dz_ode.h, INPUTS)."""
    L, tests = [], _finite(_indices_read([g for _, g in net.inputs if g is not None]))
    for i, (_, gain) in enumerate(net.inputs):
        L.append("        k[%d] = %s;" % (first + i, "1.0" if gain is None else net.constant(gain)[0]))
        if gain is not None:
            tests += _finite((), ["k[%d]" % (first + i)]) + ["k[%d] > 0.0" % (first + i)]
    return L, tests


def _input_members(net, drive):
    """The members of a generated network with inputs (csrc/dz_ode.h's head, INPUTS), for the three emitters alike.  drive: the entry of
    the point's values at which the drives begin; the gains stand in front of them."""
    I = len(net.inputs)
    species, scaled = "-1", "v"
    for i in reversed(range(I)):
        species = "i == %d ? %d : %s" % (i, net.inputs[i][0], species)
        if net.inputs[i][1] is not None:
            scaled = "i == %d ? k[%d] * v : %s" % (i, drive - I + i, scaled)
    L = ["    static constexpr int INPUTS = %d, DRIVE = %d;" % (I, drive),
         "    DZO_HD static int input_species(int i) { return %s; }" % species,
         "    DZO_HD static double input_scaled(int i, const double* k, double v) { return %s; }" % scaled]
    if net.lanes != 1:                      # (the group form: gain i by lane (R + SLOTS + i) % L once per point)
        L += ["    DZO_HD static double gain(int i, const double* x, bool& good)", "    {", "        switch (i) {"]
        for i, (_, gain) in enumerate(net.inputs):
            if gain is not None:
                value, idx = net.constant(gain)
                L.append("        case %d: { const double v = %s; good = %s; return v; }" % (i, value, " && ".join(_finite(idx, ["v"]) + ["v > 0.0"])))
        L += ["        default: good = true; return 1.0;", "        }", "    }"]
    return L


def _monomial_members(mono):
    """The members of a generated network that has monomials (csrc/dz_ode.h's head), for the one-lane and the lane-group source alike.
    mono: dict(y0={species: Monomial}, scale=[float | Monomial] or None, constraints=[(Monomial, loc, sd)])."""
    y0, scale, cons = mono["y0"], mono["scale"] or [], mono["constraints"]
    outside = [m for _, m in sorted(y0.items())] + [f for f in scale if isinstance(f, Monomial)] + [m for m, _, _ in cons]
    tests = _finite(_indices_read(outside), [_mono_value(m) for m in outside])
    L = ["    static constexpr bool MONOMIALS = true;", "    DZO_HD static bool live(const double* x)", "    {",
         "        return %s;" % (" && ".join(tests) or "true"), "    }",
         "    DZO_HD static double y0_row(int r, const double* x, double b)", "    {"]
    if y0:
        L += ["        const double m%d = %s;" % (s, _mono_value(m)) for s, m in sorted(y0.items())]
        sel = "0.0"
        for s in sorted(y0, reverse=True):
            sel = "r == %d ? m%d : %s" % (s, s, sel)
        L += ["        const double m = %s;" % sel, "        return b != b ? m : b;"]
    else:
        L.append("        return b;")
    L += ["    }", "    DZO_HD static void scale(const double* x, double* o)", "    {"]
    L += ["        o[%d] = %s * o[%d];" % (q, _mono_value(f) if isinstance(f, Monomial) else _hexlit(f), q) for q, f in enumerate(scale) if f != 1.0]
    L.append("    }")
    if cons:
        G0 = float(sum(-np.log(sd) - _LOG_2PI_HALF for _, _, sd in cons))
        L += ["    DZO_HD static double constraints(const double* x)", "    {", "        double acc = 0.0;"]
        L += ["        { const double r = (%s - %s) / %s; acc = acc - 0.5 * r * r; }" % (_mono_value(m), _hexlit(loc), _hexlit(sd)) for m, loc, sd in cons]
        L += ["        return %s + acc;" % _hexlit(G0), "    }"]
    return L


def _noise_members(net):
    """The members of a generated network with sampled noise (csrc/dz_ode.h's head, NOISE), for the three emitters alike: the per-point
    values a_q, b_q with their liveness, and one output time's terms with q a constant.  net.noise: O entries, None or a Noise."""
    L = ["    static constexpr bool NOISE = true;", "    DZO_HD static double noise_value(int m, const double* x, bool& good)", "    {", "        switch (m) {"]
    for q, z in enumerate(net.noise):
        for m, c, bound in ((2 * q, z and z.sigma, "v > 0.0"), (2 * q + 1, z and z.rel, "v >= 0.0")):
            if c is not None:
                value, idx = net.constant(c)
                L.append("        case %d: { const double v = %s; good = %s; return v; }" % (m, value, " && ".join(_finite(idx, ["v"]) + [bound])))
            elif z is not None:             # (a Noise without rel: b = 0; an observable without a Noise: NaN, below)
                L.append("        case %d: good = true; return 0.0;" % m)
    L += ['        default: good = true; return __builtin_nan("");', "        }", "    }",
          "    DZO_HD static bool noise_terms(const double* nz, const double* o, const double* dat, const double* sd, double& acc)", "    {",
          "        bool good = true;"]
    for q, z in enumerate(net.noise):
        if net.normalize and net.normalize[q] is not None:      # (csrc/dz_ode.h, NORMALISED READOUTS: its terms come behind the last row)
            continue
        if z is None:                       # (the two statements this observable always ran)
            L.append("        { const double r = (o[%d] - dat[%d]) / sd[%d]; acc = acc - 0.5 * r * r; }" % (q, q, q))
            continue
        log = z.scale == "log"
        L += ["        {", "            const double m = o[%d], w = sd[%d];" % (q, q),
              "            double s = nz[%d]%s;" % (2 * q, " + nz[%d] * dzode::dabs(m)" % (2 * q + 1) if z.rel is not None else ""),
              "            s = s * w;",
              "            const double r = (%s - dat[%d]) / s;" % ("dzode::dlog(m)" if log else "m", q),
              "            double a = acc - %s;" % ("0.5 * r * r" if z.dist == "normal" else "dzode::dabs(r)"),
              "            a = a - dzode::dlog(s);",
              "            const bool seen = w < __builtin_huge_val();",
              "            acc = seen ? a : acc;",
              "            good = good && (!seen || (dzode::finite(m) && %sdzode::finite(s) && s > 0.0));" % ("m > 0.0 && " if log else ""),
              "        }"]
    return L + ["        return good;", "    }"]


_NORM_KINDS = {"max": 1, "ref": 2, "minmax": 3}      # the record's first double
_NORM_RECORD = 7                                      # kind, reference row, D, E, W, n_q, L_q


def _normalize_members(net):
    """The members of a generated network with normalised readouts (csrc/dz_ode.h's head, NORMALISED READOUTS), for the three emitters
    alike, with q a constant.  Normalised observable number i (ascending q) reads record i of the block, rec[7 i ..], and owns the
    accumulators na[b ..]: "max" and "ref" the sums A, B and the value g; "minmax" the sums A, B, C and the values hi, lo."""
    entries = [(q, z) for q, z in enumerate(net.normalize) if z is not None]
    base, b = [], 0
    for _, z in entries:
        base.append(b)
        b += 5 if z.kind == "minmax" else 3
    L = ["    static constexpr int NORMALIZE = %d, NORM_KNOTS = %d, NORM_ACC = %d;" % (len(entries), net.knots, b),
         "    DZO_HD static bool normalized(int q) { return %s; }" % " || ".join("q == %d" % q for q, _ in entries),
         "    DZO_HD static void norm_init(double* na)", "    {"]
    for (q, z), b in zip(entries, base):
        L += ["        na[%d] = 0.0;" % (b + m) for m in range(3 if z.kind == "minmax" else 2)]
        if z.kind == "minmax":
            L += ["        na[%d] = -__builtin_huge_val();" % (b + 3), "        na[%d] = __builtin_huge_val();" % (b + 4)]
        else:
            L.append("        na[%d] = %s;" % (b + 2, "-__builtin_huge_val()" if z.kind == "max" else "0.0"))
    L += ["    }", "    DZO_HD static void norm_accumulate(const double* rec, int j, const double* o, const double* dat, const double* sd, double* na)", "    {"]
    for i, ((q, z), b) in enumerate(zip(entries, base)):
        L += ["        {", "            const double m = o[%d], iw = 1.0 / sd[%d];" % (q, q),
              "            const double p = m * iw, e = dat[%d] * iw;" % q,
              "            na[%d] = na[%d] + p * p;" % (b, b), "            na[%d] = na[%d] + p * e;" % (b + 1, b + 1)]
        if z.kind == "max":
            L.append("            na[%d] = m > na[%d] ? m : na[%d];" % (b + 2, b + 2, b + 2))
        elif z.kind == "ref":
            L.append("            na[%d] = j == (int)rec[%d] ? m : na[%d];" % (b + 2, _NORM_RECORD * i + 1, b + 2))
        else:
            L += ["            na[%d] = na[%d] + p * iw;" % (b + 2, b + 2), "            na[%d] = m > na[%d] ? m : na[%d];" % (b + 3, b + 3, b + 3),
                  "            na[%d] = m < na[%d] ? m : na[%d];" % (b + 4, b + 4, b + 4)]
        L.append("        }")
    L += ["    }", "    DZO_HD static bool norm_finish(const double* rec, const double* nz, const double* na, double& acc)", "    {", "        bool good = true;"]
    for i, ((q, z), b) in enumerate(zip(entries, base)):
        r = _NORM_RECORD * i
        L.append("        {")
        if z.kind == "minmax":
            L += ["            const double lo = na[%d], g = na[%d] - lo;" % (b + 4, b + 3),
                  "            const double A = na[%d] - 2.0 * (lo * na[%d]) + (lo * lo) * rec[%d];" % (b, b + 2, r + 4),
                  "            const double B = na[%d] - lo * rec[%d];" % (b + 1, r + 3)]
        else:
            L.append("            const double g = na[%d], A = na[%d], B = na[%d];" % (b + 2, b, b + 1))
        L += ["            const double z = 1.0 / g;", "            const double Q = (A * z) * z - 2.0 * (B * z) + rec[%d];" % (r + 2)]
        if net.noise and net.noise[q] is not None:
            L += ["            const double a = nz[%d];" % (2 * q), "            acc = acc - (0.5 * Q) / (a * a);",
                  "            acc = acc - rec[%d] * dzode::dlog(a);" % (r + 5), "            acc = acc - rec[%d];" % (r + 6)]
        else:
            L.append("            acc = acc - 0.5 * Q;")
        L += ["            good = good && dzode::finite(g) && g > 0.0;", "        }"]
    L += ["        return good;", "    }", "    DZO_HD static void norm_apply(const double* na, double* row)", "    {"]
    for (q, z), b in zip(entries, base):
        if z.kind == "minmax":
            L.append("        row[%d] = (row[%d] - na[%d]) / (na[%d] - na[%d]);" % (q, q, b + 4, b + 3, b + 4))
        else:
            L.append("        row[%d] = row[%d] / na[%d];" % (q, q, b + 2))
    return L + ["    }"]


def _product(factors):
    return " * ".join(factors) if factors else "1.0"


def _rate_factors(reac, skip=None):
    out = []
    for s, c in sorted(reac.items()):
        out += ["y[%d]" % s] * (c - (1 if s == skip else 0))
    return out


def _combine(terms):                        # [(integer coefficient, expression)] -> a sum in this order
    out = ""
    for c, e in terms:
        t = e if abs(c) == 1 else "%d.0 * %s" % (abs(c), e)
        out += ("-" if c < 0 else "") + t if not out else (" - " if c < 0 else " + ") + t
    return out or "0.0"


def _obs_lines(S, observables):
    L = []
    for o, row in enumerate(observables):
        terms = ["y[%d]" % s if row[s] == 1.0 else "%s * y[%d]" % (_hexlit(row[s]), s) for s in range(S) if row[s] != 0.0]
        L.append("        o[%d] = %s;" % (o, " + ".join(terms) if terms else "0.0"))
    return L


def _net_source(net, body):
    """The scaffolding every generated source shares: the include, the struct's head, the generator's own members (body, up to the
    closing brace of the last one), the members of a network with inputs (net.drive: where the emitter put their drives), of one with monomials, the observables and the entry macro.  net.events: the
    largest event count over the object's experiments; the member EVENTS only if there is one (csrc/dz_ode.h).  net.equilibrate: some
    experiment equilibrates first; the member EQUILIBRATE only then.  net.settle: the object's t ends in inf; the member SETTLE only then.
    net.normalize: some observable is normalised to its own time course; NORMALIZE, norm_accumulate and norm_finish only then."""
    if net.lanes == 1:
        header, entries = "dz_ode.h", "DZODE_ITEM_ENTRIES(Net)" if net.items else "DZODE_ENTRIES(Net)"
    else:
        header, entries = "dz_ode_group.h", ("DZODE_GROUP_ITEM_ENTRIES(Net, %d)" if net.items else "DZODE_GROUP_ENTRIES(Net, %d)") % net.lanes
    L = ["struct Net {", "    static constexpr int S = %d, R = %d, O = %d;" % (net.S, net.R, len(net.observables))]
    L += ["    static constexpr int EVENTS = %d;" % net.events] if net.events else []
    L += ["    static constexpr bool EQUILIBRATE = true;"] if net.equilibrate else []
    L += ["    static constexpr bool SETTLE = true;"] if net.settle else []
    L += ["    static constexpr int VIEW = %d;" % net.view] if net.view else []
    L += _input_members(net, net.drive) if net.inputs else []
    L += body + (_monomial_members(net.mono) if net.mono else []) + (_noise_members(net) if net.noise else [])
    L += _normalize_members(net) if net.normalize else []
    L += ["    DZO_HD static void obs(const double* y, double* o)", "    {"] + _obs_lines(net.S, net.observables) + ["    }", "};", entries, ""]
    return '#include "%s"\n' % header + "\n".join(L)


_ODE_WHOLE_SUMS = 16        # up to this many reactions the one-lane source names every rate and writes each f[s] and J[i] as one sum


def _ode_long_source(net):
    """The one-lane source for more than _ODE_WHOLE_SUMS reactions.  Every f[s] and J[i] is the same sum in the same (ascending reaction)
    order as in the short form, but built up reaction by reaction, so one rate is live at a time and not all R; DZODE_FENCE between the
    reactions keeps the compiler from starting them all at once (see csrc/dz_ode.h).  k holds one rate constant per parameter that is
    used, not one per reaction, and a fixed rate constant is a literal where it is used: what stays in registers through the
    integration is the number of distinct parameters."""
    S, N = net.S, net.N
    used = sorted({rate for rate in net.rates if isinstance(rate, _INT)})
    for rate in net.rates:                      # (then a slot per distinct monomial, in the order of their first reactions)
        if isinstance(rate, Monomial) and rate not in used:
            used.append(rate)
    kname = ["k[%d]" % used.index(rate) if isinstance(rate, _INT + (Monomial,)) else _hexlit(rate) for rate in net.rates]
    v, dv = net.rate_code(kname, len(used))
    slot_lines, slot_tests = _slot_lines(net, len(used))    # (then the Hill slots: k[len(used) + m] = Kn)
    gain_lines, gain_tests = _input_lines(net, len(used) + len(net.slots))     # (then the inputs' gains and, behind them, their drives)
    net.drive = len(used) + len(net.slots) + len(net.inputs)
    started = set()

    def add(target, c, e):
        t = e if abs(c) == 1 else "%d.0 * %s" % (abs(c), e)
        if target in started:
            return "        %s = %s %s %s;" % (target, target, "-" if c < 0 else "+", t)
        started.add(target)
        return "        %s = %s%s;" % (target, "-" if c < 0 else "", t)

    L = ["    static constexpr int SLOTS = %d;" % len(net.slots)] if net.slots else []
    L += ["    DZO_HD static bool rates(const double* x, double* k)", "    {"]
    L += ["        k[%d] = %s;" % (i, net.constant(p)[0]) for i, p in enumerate(used)]
    L += slot_lines + gain_lines
    L.append("        return %s;" % (" && ".join(_finite(_rate_indices(net.reactions), ["k[%d]" % i for i in range(len(used))]) + slot_tests + gain_tests) or "true"))
    L += ["    }", "    DZO_HD static void rhs(const double* k, const double* y, double* f)", "    {"]
    for r in range(net.R):
        rows = [s for s in range(S) if N[s, r] != 0]
        if not rows:
            continue
        L.append("        const double v%d = %s;" % (r, v(r)))
        L += [add("f[%d]" % s, int(N[s, r]), "v%d" % r) for s in rows]
        L.append("        " + " ".join("DZODE_FENCE(f[%d]);" % s for s in rows))
    # (a species no reaction changes: 0, or for an input species its drive)
    L += ["        f[%d] = %s;" % (s, "0.0" if net.input_of(s) is None else "k[%d]" % (net.drive + net.input_of(s))) for s in range(S) if "f[%d]" % s not in started]
    L += ["    }", "    DZO_HD static void jac(const double* k, const double* y, double* J)", "    {"]
    for r in range(net.R):                              # dv_r / dy_q = k nu_q y_q^(nu_q - 1) prod_others y^nu (a RateLaw: rate_code's dv)
        rows = [s for s in range(S) if N[s, r] != 0]
        for q in net.kinetic[r]:
            if not rows:
                continue
            L.append("        const double d%d_%d = %s;" % (r, q, dv(r, q)))
            L += [add("J[%d]" % (s * S + q), int(N[s, r]), "d%d_%d" % (r, q)) for s in rows]
            L.append("        " + " ".join("DZODE_FENCE(J[%d]);" % (s * S + q) for s in rows))
    L += ["        J[%d] = 0.0;" % i for i in range(S * S) if "J[%d]" % i not in started]
    return _net_source(net, L + ["    }"])


def _ode_source(net):
    """The generated network struct (see csrc/dz_ode.h; the scaffolding around it: _net_source): rate constants, right-hand side, analytic Jacobian and observables as
    straight-line code with constant indices; powers as repeated products.  net.items: the entry points for several conditions per point."""
    S, R, N = net.S, net.R, net.N
    if R > _ODE_WHOLE_SUMS:
        return _ode_long_source(net)
    v, dv = net.rate_code(["k[%d]" % r for r in range(R)], R)
    slot_lines, slot_tests = _slot_lines(net, R)        # (the Hill slots behind the rate constants: k[R + m] = Kn)
    gain_lines, gain_tests = _input_lines(net, R + len(net.slots))      # (then the inputs' gains and, behind them, their drives)
    net.drive = R + len(net.slots) + len(net.inputs)
    L = ["    static constexpr int SLOTS = %d;" % len(net.slots)] if net.slots else []
    L += ["    DZO_HD static bool rates(const double* x, double* k)", "    {"]
    L += ["        k[%d] = %s;" % (r, net.constant(rate)[0]) for r, rate in enumerate(net.rates)]
    L += slot_lines + gain_lines                # (10**-inf is a finite 0: test x itself)
    L.append("        return %s;" % " && ".join(_finite(_rate_indices(net.reactions), ["k[%d]" % r for r in range(R)]) + slot_tests + gain_tests))
    L += ["    }", "    DZO_HD static void rhs(const double* k, const double* y, double* f)", "    {"]
    L += ["        const double v%d = %s;" % (r, v(r)) for r in range(R)]
    for s in range(S):
        if net.input_of(s) is not None:                 # (an input species: its drive; nothing produces or consumes it)
            L.append("        f[%d] = k[%d];" % (s, net.drive + net.input_of(s)))
            continue
        L.append("        f[%d] = %s;" % (s, _combine([(int(N[s, r]), "v%d" % r) for r in range(R) if N[s, r] != 0])))
    L += ["    }", "    DZO_HD static void jac(const double* k, const double* y, double* J)", "    {"]
    for r in range(R):                                  # dv_r / dy_q = k nu_q y_q^(nu_q - 1) prod_others y^nu (a RateLaw: rate_code's dv)
        L += ["        const double d%d_%d = %s;" % (r, q, dv(r, q)) for q in net.kinetic[r]]
    for s in range(S):
        for q in range(S):
            terms = [(int(N[s, r]), "d%d_%d" % (r, q)) for r in range(R) if N[s, r] != 0 and q in net.kinetic[r]]
            L.append("        J[%d] = %s;" % (s * S + q, _combine(terms)))
    return _net_source(net, L + ["    }"])


def _ode_group_source(net):
    """The generated network struct for the lane-group solver and, with lanes=64, the wave-per-point one (csrc/dz_ode_group.h).  Lane r (or the host build's loop iteration r) gets
    its own f[r] and J[r][q] WITHOUT a branch on r: every reaction's rate is evaluated by every lane and multiplied by that lane's
    stoichiometric coefficient, a select over constants (0 for a species the reaction does not touch), so the lanes of a wave never
    diverge inside the right-hand side.  Every f[r] and J[r][q] is the sum over the reactions (for J: those with q among the reactants)
    in ascending reaction index of coefficient(r) * (k[j] * (nu) * y...) -- written here once, compiled for both sides."""
    S, R, N = net.S, net.R, net.N

    def coefficient(j):                     # N[r][j] as a function of r
        out = "0.0"
        for s in reversed([s for s in range(S) if N[s, j] != 0]):
            out = "r == %d ? %d.0 : %s" % (s, N[s, j], out)
        return "(%s)" % out

    def weighted_sum(terms, indent):        # [(j, expression)] -> statements that leave the sum in v
        if not terms:
            return [indent + "return 0.0;"]
        out = [indent + "int z = 0;", indent + "double v = %s * (%s);" % (coefficient(terms[0][0]), terms[0][1])]
        for t, (j, e) in enumerate(terms[1:], 1):
            if t % 4 == 0:                  # (a long sum in groups of four terms: see DZODE_SUM_FENCE in csrc/dz_ode_group.h)
                out.append(indent + "DZODE_SUM_FENCE(v, r, z);")
            out.append(indent + "v = v + %s * (%s);" % (coefficient(j), e))
        return out + [indent + "return v;"]

    # (the Hill slots behind the rate constants: k[R + m] = Kn, by lane (R + m) % L once per point)
    v, dv = net.rate_code(["k[z + %d]" % j for j in range(R)], R)
    net.drive = R + len(net.slots) + len(net.inputs)    # (behind the slots the inputs' gains, then their drives: csrc/dz_ode_group.h)
    sampled = _INT + (Monomial,)
    L = ["    static constexpr bool LOG10 = %s;" % ("true" if net.log10 else "false"),
         "    DZO_HD static int rate_index(int j)", "    {", "        switch (j) {"]
    L += ["        case %d: return %d;" % (j, -2 if isinstance(rate, Monomial) else rate) for j, rate in enumerate(net.rates) if isinstance(rate, sampled)]
    L += ["        default: return -1;", "        }", "    }", "    DZO_HD static double rate_fixed(int j)", "    {", "        switch (j) {"]
    L += ["        case %d: return %s;" % (j, _hexlit(rate)) for j, rate in enumerate(net.rates) if not isinstance(rate, sampled)]
    L += ["        default: return 0.0;", "        }", "    }"]
    if net.slots:
        L += ["    static constexpr int SLOTS = %d;" % len(net.slots), "    DZO_HD static double slot(int m, const double* x, bool& good)", "    {", "        switch (m) {"]
        for (_, K, n), m in net.slots.items():
            kv, idx = net.constant(K)
            L.append("        case %d: { const double K = %s; const double v = %s; good = %s; return v; }"
                     % (m, kv, " * ".join(["K"] * n), " && ".join(_finite(idx, ["K", "v"]) + ["v > 0.0"])))
        L += ["        default: good = false; return 0.0;", "        }", "    }"]
    if net.mono:                                         # (rate_index -2: the reaction's own expression, by lane j % L once per point)
        L += ["    DZO_HD static double rate_mono(int j, const double* x, bool& good)", "    {", "        switch (j) {"]
        for j, rate in enumerate(net.rates):
            if isinstance(rate, Monomial):
                kv, idx = net.constant(rate)
                L.append("        case %d: { const double v = %s; good = %s; return v; }" % (j, kv, " && ".join(_finite(idx, ["v"]))))
        L += ["        default: good = false; return 0.0;", "        }", "    }"]
    L += ["    DZO_HD static double rhs_row(int r, const double* k, const double* y)", "    {"]
    row = weighted_sum([(j, v(j)) for j in range(R) if np.any(N[:, j] != 0)], "        ")
    if net.inputs:                                       # (an input's row: a select onto its drive, branch-free on the row)
        value = row.pop().strip()[len("return "):-1]
        for i, (s, _) in enumerate(net.inputs):
            value = "r == %d ? k[%d] : %s" % (s, net.drive + i, value)
        row.append("        return %s;" % value)
    L += row
    L += ["    }", "    DZO_HD static double jac_entry(int r, int q, const double* k, const double* y)", "    {", "        switch (q) {"]
    for q in range(S):                                   # dv_j / dy_q = k nu_q y_q^(nu_q - 1) prod_others y^nu
        terms = [(j, dv(j, q)) for j in range(R) if q in net.kinetic[j] and np.any(N[:, j] != 0)]
        L += ["        case %d: {" % q] + weighted_sum(terms, "            ") + ["        }"]
    return _net_source(net, L + ["        default: return 0.0;", "        }", "    }"])


def generate(like):
    """The source of a checked MassActionODELogLike: the one-lane struct, or the lane group's."""
    net = _Network(like)
    return _ode_source(net) if net.lanes == 1 else _ode_group_source(net)
