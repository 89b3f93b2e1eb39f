"""QueryIdentity rows steered onto the edges of the device's integer shortcuts, for TD3 and TD1. Plain Python: no
GPU, no oracle.

The device does not port the circuit's comparators, date templates and SMT state machine template by template: it
restates them over integers (csrc/query.hpp q_v64, the RK_Q_CMP regions, q_dil_sig, q_ediln_sig, k_qry_prep's
status; csrc/regcore.hpp k_smt_prep's lev / done recurrences over the gathered isZero mask). pzkwit.query.make_query
draws avoid every edge of those shortcuts: no empty sibling inside a proof, no bound equal to its value, no 0 or
2^64 - 1, no two dates that share a year, no failing condition but one. Every row here starts from a make_query
query with a fixed seed per case and rebuilds what its edit invalidates (the identity state's value and root; for a
DG1 date also the DG1 bits, the commitment and the extracted field).

features() restates, in integers, the decisions the device code takes and names those a row reaches;
tests/test_query_cases.py requires the committed rows to reach all of FEATURES and pins the oracle and the
constraint checker on every row, tests/test_gpu_query_cases.py compares the device.

Groups: smt (isZero masks, all valid proofs), cmp64 (the four 64-bit comparisons), date (the four date
comparisons), select (each selector bit alone), domain (an input equal to 2^64: outside the evaluated domain).

Year differences: the years DateIsLess compares are at most 100 apart, not 199 as two-digit years + 100 suggest.
The normalisation adds 100 to a year exactly when its date is before currentDate in (year, month, day) order, so
the two bits differ only when currentDate lies between the dates: n1 = 1, n2 = 0 means first < currentDate <=
second, hence y1 <= y2 and ya - yb = 100 + y1 - y2 <= 100 (and >= 1); n1 = 0, n2 = 1 gives [-100, -1]; equal bits
give [-99, 99] for digit years. The rows *_year_plus_100 / *_year_minus_100 sit on that bound."""
import hashlib

from pzkwit import query as Q
from pzkwit.field import SplitMix64, poseidon

# csrc/layout.hpp: "constexpr int SMT_LEVELS = 80;" and "constexpr int SMT_PREP_LANES = 8;  // k_smt_prep: lanes per
# witness (10 levels each)"; regcore.hpp k_smt_prep: NL = SMT_LEVELS / SMT_PREP_LANES
SMT_LEVELS, SMT_PREP_LANES = 80, 8
NL = SMT_LEVELS // SMT_PREP_LANES
M64 = (1 << 64) - 1
ST_NUM2BITS, ST_QUERY, ST_DATE, ST_INPUT_RANGE = 1, 19, 20, 64
CUR, CUR_PREV, CUR_NEXT = b"241017", b"241016", b"241018"  # make_query's currentDate and its neighbours
ALL = (1 << 18) - 1
GROUPS = ("smt", "cmp64", "date", "select", "domain")

# the eight ForceEqualIfEnabled conditions (queryIdentity.circom:109-188), selector bit 8 + k
COND = ("timestamp >= lower", "timestamp < upper", "counter >= lower", "counter < upper", "expiration lower < date",
        "expiration date < upper", "birth lower < date", "birth date < upper")
CMP = (("timestamp", "timestampLowerbound"), ("timestamp", "timestampUpperbound"),
       ("identityCounter", "identityCounterLowerbound"), ("identityCounter", "identityCounterUpperbound"))
DATE_BOUND = {4: "expirationDateLowerbound", 5: "expirationDateUpperbound", 6: "birthDateLowerbound",
              7: "birthDateUpperbound"}
DILS = ("edlo", "edhi", "bdlo", "bdhi", "bdlo_n1", "bdlo_n2", "bdhi_n1", "bdhi_n2")
# bit offset of the dates in dg1 (DG1DataExtractor / DG1TD1DataExtractor), and their index in info["fields"]
DATE_BIT = {False: {"birth": 496, "exp": 560}, True: {"birth": 280, "exp": 344}}
DATE_FIELD = {"birth": 0, "exp": 1}

FEATURES = tuple(
    ["cmp%d_%s" % (k, f) for k in range(4) for f in ("borrow", "no_borrow", "v64_set", "v64_clear")] +
    ["cmp0_carry", "cmp2_carry"] +
    ["%s_%s" % (d, f) for d in DILS for f in ("yl", "ml", "dl", "none", "ydiff_pos", "ydiff_neg", "mdiff_pos",
                                                "mdiff_neg")] +
    ["%s_ydiff_%s_100" % (d, g) for d in ("bdlo", "bdhi") for g in ("plus", "minus")] +
    ["%s_norm_%d%d" % (d, a, b) for d in ("bdlo", "bdhi") for a in (0, 1) for b in (0, 1)] +
    ["cond%d_false_%s" % (k, s) for k in range(8) for s in ("selected", "unselected")] +
    ["smt_interior_zero", "smt_zero_level_0", "smt_zero_lane_first", "smt_zero_lane_last", "smt_zero_word_first",
     "smt_zero_word_last", "smt_zero_run", "smt_lev79", "smt_j_0", "smt_j_1", "smt_j_79", "smt_keybit_j_0",
     "smt_keybit_j_1"] +
    ["smt_single_zero_%d" % z for z in (0, NL - 1, NL, 2 * NL - 1, 31, 32, 63, 64, 77)] +
    ["smt_only_top_sibling", "smt_only_end_siblings", "smt_alternating_even", "smt_alternating_odd"])


def enc(date):
    """b"YYMMDD" -> the encoded date"""
    assert len(date) == 6
    return int.from_bytes(date, "big")


def decode(e):
    """(year, month, day) as DateDecoder's nibble reads give them (q_dec)"""
    return (((e >> 40) & 15) * 10 + ((e >> 32) & 15), ((e >> 24) & 15) * 10 + ((e >> 16) & 15),
            ((e >> 8) & 15) * 10 + (e & 15))


def date_less(a, b):
    """DateIsLess.out on (year, month, day) triples"""
    return int(a < b)


def _dil_features(name, a, b):
    f = {"%s_%s" % (name, "yl" if a[0] < b[0] else "ml" if a[:1] == b[:1] and a[1] < b[1] else
                    "dl" if a[:2] == b[:2] and a[2] < b[2] else "none")}
    for tag, d in (("ydiff", b[0] - a[0]), ("mdiff", b[1] - a[1])):  # the IsEqual differences second - first
        if d:
            f.add("%s_%s_%s" % (name, tag, "pos" if d > 0 else "neg"))
    if abs(b[0] - a[0]) >= 100 and name in ("bdlo", "bdhi"):  # the bound of a normalised pair (module docstring)
        f.add("%s_ydiff_%s_100" % (name, "plus" if b[0] > a[0] else "minus"))
    return f


def insertion_level(siblings):
    j = len(siblings)
    while j > 0 and siblings[j - 1] == 0:
        j -= 1
    return j


def conditions(inp, info):
    """the eight conditions, on in-domain inputs"""
    birth, exp, cur = info["fields"][0], info["fields"][1], decode(inp["currentDate"])

    def norm(e):
        y, m, d = decode(e)
        return (y + 100 * date_less((y, m, d), cur), m, d)

    ts, ic = inp["timestamp"], inp["identityCounter"]
    return [int(ts >= inp["timestampLowerbound"]), int(ts < inp["timestampUpperbound"]),
            int(ic >= inp["identityCounterLowerbound"]), int(ic < inp["identityCounterUpperbound"]),
            date_less(decode(inp["expirationDateLowerbound"]), decode(exp)),
            date_less(decode(exp), decode(inp["expirationDateUpperbound"])),
            date_less(norm(inp["birthDateLowerbound"]), norm(birth)),
            date_less(norm(birth), norm(inp["birthDateUpperbound"]))]


def features(inp, info):
    """labels of the decisions query.hpp and k_smt_prep take on a row; a subset of FEATURES. A row with an input
    read as a 64-bit integer that is >= 2^64 reaches none: the device flags it before it decides anything."""
    u64 = [n for n in Q.NAMES[4:13]] + ["timestamp", "identityCounter"]
    if any(inp[n] > M64 for n in u64):
        return set()
    f = set()
    for k, (xn, yn) in enumerate(CMP):
        x, y = inp[xn], inp[yn]
        if k & 1:  # LessThan(64)(x, y): v = x + 2^64 - y, q_v64(x, 0, y, 0)
            borrow, v = x < y, x + (1 << 64) - y
        else:      # GreaterEqThan(64): LessThan(64)(y, x + 1): v = y + 2^64 - (x + 1), q_v64(y, 0, x1, x1h)
            x1 = (x + 1) & M64
            if x1 == 0:
                f.add("cmp%d_carry" % k)
            borrow, v = y < x1, y + (1 << 64) - (x + 1)
        assert 0 <= v < 1 << 65
        f.add("cmp%d_%s" % (k, "borrow" if borrow else "no_borrow"))
        f.add("cmp%d_%s" % (k, "v64_set" if v >> 64 else "v64_clear"))
    birth, exp, cur = decode(info["fields"][0]), decode(info["fields"][1]), decode(inp["currentDate"])
    f |= _dil_features("edlo", decode(inp["expirationDateLowerbound"]), exp)
    f |= _dil_features("edhi", exp, decode(inp["expirationDateUpperbound"]))
    for name, a, b in (("bdlo", decode(inp["birthDateLowerbound"]), birth),
                       ("bdhi", birth, decode(inp["birthDateUpperbound"]))):
        n1, n2 = date_less(a, cur), date_less(b, cur)
        f |= _dil_features(name + "_n1", a, cur) | _dil_features(name + "_n2", b, cur)
        f.add("%s_norm_%d%d" % (name, n1, n2))
        f |= _dil_features(name, (a[0] + 100 * n1,) + a[1:], (b[0] + 100 * n2,) + b[1:])
    for k, c in enumerate(conditions(inp, info)):
        if not c:
            f.add("cond%d_false_%s" % (k, "selected" if (inp["selector"] >> (8 + k)) & 1 else "unselected"))
    sib = inp["idStateSiblings"]
    j = insertion_level(sib)
    zeros = [i for i in range(j) if sib[i] == 0]  # empty siblings inside the path
    if zeros:
        f.add("smt_interior_zero")
    if 0 in zeros:
        f.add("smt_zero_level_0")
    if any(i and i % NL == 0 for i in zeros):
        f.add("smt_zero_lane_first")
    if any(i % NL == NL - 1 for i in zeros):
        f.add("smt_zero_lane_last")
    if any(i and i % 32 == 0 for i in zeros):
        f.add("smt_zero_word_first")
    if any(i % 32 == 31 for i in zeros):
        f.add("smt_zero_word_last")
    if any(i + 1 in zeros for i in zeros):
        f.add("smt_zero_run")
    if len(zeros) == 1 and "smt_single_zero_%d" % zeros[0] in FEATURES:
        f.add("smt_single_zero_%d" % zeros[0])
    if j == SMT_LEVELS - 1 and zeros == list(range(j - 1)):
        f.add("smt_only_top_sibling")
    if j == SMT_LEVELS - 1 and zeros == list(range(1, j - 1)):
        f.add("smt_only_end_siblings")
    if len(zeros) > 1 and zeros == list(range(zeros[0], j, 2)) and zeros[0] < 2:
        f.add("smt_alternating_%s" % ("odd" if zeros[0] else "even"))
    if sib[SMT_LEVELS - 2]:
        f.add("smt_lev79")
    if j in (0, 1, 79):
        f.add("smt_j_%d" % j)
    f.add("smt_keybit_j_%d" % ((info["key"] >> j) & 1))
    return f


# ---- rebuilding what an edit invalidates
def reroot(inp, info):
    """after timestamp, identityCounter, the commitment or the siblings changed"""
    info["value"] = poseidon([info["dg_commit"], inp["identityCounter"], inp["timestamp"]])
    inp["idStateRoot"] = Q.smt_root(info["key"], info["value"], inp["idStateSiblings"])


def set_dg1_date(inp, info, which, date):
    """write the six bytes of the DG1's birth / expiration date, then the chunks, the commitment, the extracted
    field and the root (as make_query builds them)"""
    td1 = info["td1"]
    bits = list(inp["dg1"])
    o = DATE_BIT[td1][which]
    for i, byte in enumerate(date):
        for b in range(8):
            bits[o + 8 * i + b] = (byte >> (7 - b)) & 1
    inp["dg1"] = bits
    ch = 190 if td1 else 186
    chunks = [sum(bits[ch * i + j] << j for j in range(ch)) for i in range(4)]
    info["dg_commit"] = poseidon(chunks + [poseidon([inp["skIdentity"]])])
    info["fields"] = list(info["fields"])
    info["fields"][DATE_FIELD[which]] = enc(date)
    reroot(inp, info)


class Case:
    """name; group; inp, info: as make_query returns them, edited; code: the oracle's check-site code; device: the
    device's status (the same but in the domain group); edits: the inputs the case changed (the root follows);
    made: make_query's arguments for the unedited query"""

    def __init__(self, name, group, inp, info, code, edits, made, device=None):
        self.name, self.group, self.inp, self.info, self.code = name, group, inp, info, code
        self.edits, self.made = frozenset(edits), made
        self.device = code if device is None else device

    def __repr__(self):
        return "Case(%s)" % self.name


def seed_of(name):
    return int.from_bytes(hashlib.sha256(("query_cases " + name).encode()).digest()[:8], "big")


def unedited(case, td1):
    return Q.make_query(SplitMix64(case.made["seed"]), depth=case.made["depth"], selector=case.made["selector"],
                        td1=td1)


_CASES = {}


def cases(td1):
    """The committed rows of one document type, in order (built once per process)."""
    td1 = bool(td1)
    if td1 in _CASES:
        return _CASES[td1]
    out = []

    def mk(name, depth=None, selector=None):
        made = {"seed": seed_of(name), "depth": depth, "selector": selector}
        inp, info = Q.make_query(SplitMix64(made["seed"]), depth=depth, selector=selector, td1=td1)
        inp["idStateSiblings"] = list(inp["idStateSiblings"])
        return inp, info, made

    def add(name, group, inp, info, code, edits, made, device=None):
        out.append(Case(name, group, inp, info, code, edits, made, device))

    def bit(k):
        return 1 << (8 + k)

    # ---------------------------------------------------------------- smt: isZero masks, all valid proofs
    def smt_row(name, depth, zeros=()):
        inp, info, made = mk(name, depth=depth)
        for z in zeros:
            assert z < depth and inp["idStateSiblings"][z]
            inp["idStateSiblings"][z] = 0
        if zeros:
            reroot(inp, info)
        add(name, "smt", inp, info, 0, {"idStateSiblings"} if zeros else (), made)

    for z in (0, NL - 1, NL, 2 * NL - 1, 31, 32):   # a lane segment's edges; the word edge of levm / donem
        smt_row("smt_zero_%d" % z, 40, (z,))
    for z in (63, 64, 77):
        smt_row("smt_zero_%d" % z, 79, (z,))
    smt_row("smt_only_78", 79, range(78))
    smt_row("smt_zero_1_to_77", 79, range(1, 78))
    smt_row("smt_alternating_from_0", 79, range(0, 79, 2))
    smt_row("smt_alternating_from_1", 79, range(1, 79, 2))
    smt_row("smt_depth_1", 1)
    smt_row("smt_depth_2", 2)
    for want in (0, 1):  # the key's bit at the insertion level: the depth is chosen for it (the key does not depend on it)
        name = "smt_keybit_%d" % want
        key = mk(name, depth=40)[1]["key"]
        depth = next(d for d in range(33, 79) if (key >> d) & 1 == want)
        smt_row(name, depth)
        assert out[-1].info["key"] == key and (key >> insertion_level(out[-1].inp["idStateSiblings"])) & 1 == want
    smt_row("smt_depth_0", 0)

    # ---------------------------------------------------------------- cmp64
    def cmp_row(name, var, code, unselect=(), value=None, **bounds):
        sel = ALL
        for k in unselect:
            sel &= ~bit(k)
        inp, info, made = mk(name, depth=2, selector=sel)
        edits = set(bounds)
        if value is not None:
            inp[var] = value(inp[var]) if callable(value) else value
            edits.add(var)
            reroot(inp, info)
        for n, v in bounds.items():
            inp[n] = v(inp[var]) if callable(v) else v
            assert 0 <= inp[n] <= M64
        add(name, "cmp64", inp, info, code, edits, made)

    for p, var, klo in (("ts", "timestamp", 0), ("ic", "identityCounter", 2)):
        lo, hi, khi = CMP[klo][1], CMP[klo + 1][1], klo + 1
        cmp_row(p + "_eq_lower", var, 0, **{lo: lambda v: v})
        cmp_row(p + "_eq_upper_minus_1", var, 0, **{hi: lambda v: v + 1})
        cmp_row(p + "_eq_upper_selected", var, ST_QUERY, **{hi: lambda v: v})
        cmp_row(p + "_eq_upper_unselected", var, 0, unselect=(khi,), **{hi: lambda v: v})
        cmp_row(p + "_eq_lower_minus_1_selected", var, ST_QUERY, **{lo: lambda v: v + 1})
        cmp_row(p + "_eq_lower_minus_1_unselected", var, 0, unselect=(klo,), **{lo: lambda v: v + 1})
        cmp_row(p + "_zero", var, 0, value=0, **{lo: 0, hi: 1})
        cmp_row(p + "_max", var, 0, unselect=(khi,), value=M64, **{lo: M64, hi: M64})
        cmp_row(p + "_lower_max_upper_0", var, 0, unselect=(klo, khi), **{lo: M64, hi: 0})
        cmp_row(p + "_upper_max", var, 0, **{hi: M64})
        a = 0x1234
        cmp_row(p + "_high_word_only", var, 0, value=lambda v: (a << 32) | (v & 0xFFFFFFFF),
                **{lo: lambda v: v - (1 << 32), hi: lambda v: v + (1 << 32)})
        cmp_row(p + "_low_word_reversed", var, 0, value=(a << 32) | 0x80000000,
                **{lo: ((a - 1) << 32) | 0xFFFFFFF0, hi: ((a + 1) << 32) | 0x10})

    # ---------------------------------------------------------------- date
    def date_row(name, k, first, second, code, selected=True, cur=None, lo_safe=None, hi_safe=None):
        """condition k on first < second (the DG1 date and its bound, both set); the same date's other bound is set
        to a value that keeps its own condition true where one exists (lo_safe / hi_safe)"""
        inp, info, made = mk(name, depth=2, selector=7 | (bit(k) if selected else 0))
        which = "exp" if k < 6 else "birth"
        bound, dg = (first, second) if k in (4, 6) else (second, first)
        set_dg1_date(inp, info, which, dg)
        edits = {"dg1", DATE_BOUND[k], DATE_BOUND[k ^ 1]}
        if cur is not None:
            inp["currentDate"] = enc(cur)
            edits.add("currentDate")
        inp[DATE_BOUND[k]] = enc(bound)
        if which == "exp":
            other = b"000101" if k == 5 else b"991231"
        else:  # in normalised order currentDate is the earliest date and the day before it the latest
            other = (lo_safe or cur or CUR) if k == 7 else (hi_safe or CUR_PREV)
        inp[DATE_BOUND[k ^ 1]] = enc(other)
        add(name, "date", inp, info, code, edits, made)

    # valid pairs; the birth pairs also walk the normalisation comparisons (each date against 241017) through
    # month-less, day-less, year-less and not-less, with both signs of their IsEqual differences
    exp_pairs = (("day_before", b"300614", b"300615"), ("same_year_month", b"301003", b"301009"),
                 ("month_less_day_greater", b"300320", b"300705"), ("year_less_rest_greater", b"291220", b"300102"))
    birth_pairs = (("day_before", b"240914", b"240915"), ("same_year_month", b"241003", b"241009"),
                   ("month_less_day_greater", b"100320", b"100705"), ("year_less_rest_greater", b"551220", b"561102"))
    for k, tag, pairs in ((4, "edlo", exp_pairs), (5, "edhi", exp_pairs), (6, "bdlo", birth_pairs),
                          (7, "bdhi", birth_pairs)):
        for what, a, b in pairs:
            date_row("%s_%s" % (tag, what), k, a, b, 0)
    # birth around currentDate. The day before it is the latest normalised date (nothing is later: the upper check
    # fails), currentDate itself the earliest (nothing is earlier: the lower check fails).
    date_row("bdlo_birth_cur_minus_1", 6, b"300101", CUR_PREV, 0)
    date_row("bdlo_birth_cur", 6, b"300101", CUR, ST_QUERY)
    date_row("bdlo_birth_cur_plus_1", 6, CUR, CUR_NEXT, 0)
    date_row("bdhi_birth_cur_minus_1", 7, CUR_PREV, b"300101", ST_QUERY)
    date_row("bdhi_birth_cur", 7, CUR, b"300101", 0, lo_safe=b"300101")  # (its lower check cannot hold: unselected)
    date_row("bdhi_birth_cur_plus_1", 7, CUR_NEXT, CUR_PREV, 0)
    for cur, prev in ((b"000101", b"000100"), (b"991231", b"991230")):
        date_row("bdlo_cur_%s" % cur.decode(), 6, b"500101", b"600101", 0, cur=cur, hi_safe=prev)
        date_row("bdhi_cur_%s" % cur.decode(), 7, b"600101", b"701231", 0, cur=cur)
    # the largest normalised year differences (see the module docstring)
    date_row("bdlo_year_plus_100", 6, CUR, CUR_PREV, 0)
    date_row("bdlo_year_minus_100", 6, CUR_PREV, CUR, 0, selected=False, hi_safe=b"300101")
    date_row("bdhi_year_plus_100", 7, CUR, CUR_PREV, 0, lo_safe=b"300101")
    date_row("bdhi_year_minus_100", 7, CUR_PREV, CUR, 0, selected=False)
    # all-zero and all-nine bounds: digit strings, so the decoder accepts them
    date_row("bdlo_bound_000000", 6, b"000000", b"600101", 0, selected=False)
    date_row("bdlo_bound_999999", 6, b"999999", b"600101", 0, selected=False)
    date_row("bdhi_bound_000000", 7, b"600101", b"000000", 0, selected=False)
    date_row("bdhi_bound_999999", 7, b"600101", b"999999", 0, selected=False)
    # ':' in a tens place: the nibble reads give year 100, which re-encodes to ':0' again: the decoder accepts it
    date_row("edhi_bound_tens_colon", 5, b"300615", b":00101", 0)
    # failing: equality, selected and not; first later than second, not selected
    for k, tag, d in ((4, "edlo", b"300615"), (5, "edhi", b"300615"), (6, "bdlo", b"600101"), (7, "bdhi", b"600101")):
        date_row("%s_equal_selected" % tag, k, d, d, ST_QUERY)
        date_row("%s_equal_unselected" % tag, k, d, d, 0, selected=False)
    date_row("edlo_later_unselected", 4, b"310320", b"300705", 0, selected=False)
    date_row("edhi_later_unselected", 5, b"310320", b"300705", 0, selected=False)

    # a byte that is no digit: DateDecoder's re-encoding differs (20). ':' (0x3a) in a units place decodes as 10 and
    # re-encodes as a carry into the tens; in a tens place it would re-encode to itself. '?' (0x3f) everywhere.
    def nondigit(name, where, date):
        inp, info, made = mk(name, depth=2, selector=0)
        if where == "dg1":
            set_dg1_date(inp, info, "exp", date)
        else:
            inp[where] = enc(date)
        add(name, "date", inp, info, ST_DATE, {where}, made)

    nondigit("nondigit_bound_colon", "expirationDateLowerbound", b"2:0101")
    nondigit("nondigit_current_colon", "currentDate", b"24101:")
    nondigit("nondigit_dg1_colon", "dg1", b"301:15")
    nondigit("nondigit_bound_question", "birthDateUpperbound", b"??????")
    nondigit("nondigit_current_question", "currentDate", b"??????")
    nondigit("nondigit_dg1_question", "dg1", b"??????")

    # ---------------------------------------------------------------- select: each selector bit alone
    for b in range(18):
        name = "select_bit_%d" % b
        inp, info, made = mk(name, selector=1 << b)
        add(name, "select", inp, info, 0, (), made)

    # ---------------------------------------------------------------- domain: an input of 2^64 where the device reads
    # a 64-bit integer. The circuit's own answer (the oracle's code below) depends on the other inputs:
    # LessThan(64)'s Num2Bits(65) fails only when in[0] + 2^64 - in[1] leaves [0, 2^65).
    #   timestamp = 2^64              0: timestamp + 2^64 - upper and lower + 2^64 - (timestamp + 1) = lower - 1 fit;
    #                                 the upper check is false and not selected
    #   timestamp = 2^64, lower = 0   1: lower - 1 = p - 1 does not fit
    #   timestampUpperbound = 2^64    0: timestamp + 2^64 - 2^64 fits
    #   birthDateUpperbound = 2^64    20: the decoder reads nibbles of the low 48 bits (0) and re-encodes "000000"
    # The device flags such a row with 64 (PZK_ST_INPUT_RANGE) and evaluates its checks on the low 64 bits; the smallest
    # code wins. So the date bound reports the decoder's 20 (the low bits re-encode differently, as in the circuit), the
    # others 64: also where the circuit's own code, which needs the bits the device does not read, is the smaller 1 or
    # the circuit accepts the row. DESIGN.md §5 states this exception to "the smallest code".
    for name, edit, code, device in (
            ("domain_timestamp", {"timestamp": 1 << 64}, 0, ST_INPUT_RANGE),
            ("domain_timestamp_lower_0", {"timestamp": 1 << 64, "timestampLowerbound": 0}, ST_NUM2BITS, ST_INPUT_RANGE),
            ("domain_bound64", {"timestampUpperbound": 1 << 64}, 0, ST_INPUT_RANGE),
            ("domain_date_bound", {"birthDateUpperbound": 1 << 64}, ST_DATE, ST_DATE)):
        inp, info, made = mk(name, depth=2, selector=0)
        inp.update(edit)
        if "timestamp" in edit:
            reroot(inp, info)
        add(name, "domain", inp, info, code, set(edit), made, device=device)

    names = [c.name for c in out]
    assert len(names) == len(set(names))
    _CASES[td1] = out
    return out


def plain_queries(td1):
    """two plain make_query rows"""
    rng = SplitMix64(0x9C45E5 + bool(td1))
    return [Q.make_query(rng, td1=bool(td1)) for _ in range(2)]


def batch(td1, groups=GROUPS):
    """One call's rows: plain, crafted, plain, crafted, ..., plain, the plain rows alternating between the two plain
    queries. -> (input dicts, labels): labels[b] is the Case of a crafted row, 0 / 1 for a plain one."""
    plain = [inp for inp, _ in plain_queries(td1)]
    cs = [c for c in cases(td1) if c.group in groups]
    inps, labels = [], []
    for i, c in enumerate(cs):
        inps += [plain[i % 2], c.inp]
        labels += [i % 2, c]
    inps.append(plain[len(cs) % 2])
    labels.append(len(cs) % 2)
    return inps, labels
