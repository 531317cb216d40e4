"""The parameter sets of tests/test_gpu_add_forms.py, generated from the boundaries of the resident NewAdd's form selection
(make_add_params, csrc/fq_add_params.h) instead of written by hand, and the conditions they meet by construction.

A set is (gx, gy, ib); what the selection looks at is
    g = max(0, gx, gy),  shx = g - gx,  shy = g - gy,  k = g - ib.
EDGES names, for each of these and for the three arguments themselves, the values on either side of a boundary of the selection
(or of the ABI's range [-16, 16]).  For every (quantity, value) the generator takes the sets of [-16, 16]^3 at that value that
lie nearest to each of two ordinary settings (ANCHORS) in the OTHER quantities -- the edge is crossed with everything else held
as ordinary as the value allows.  The project's own sets follow: the block-tail tests' (ob3, g_res, ib) and the top-down
tests' grids x k values.

    triples()                     the list, the same for every operand-type pair and for ReLU on and off
    quantities(gx, gy, ib)        {"g": ..., "shx": ..., "shy": ..., "k": ..., "gx": ..., "gy": ..., "ib": ...}
    coverage(form_of)             what the list reaches, for the coverage tests (form_of = _native.add_resident_form)
    class_sets(form_of, xb, yb)   one set per (form, relu) class an operand-type pair can reach
    fused_sets(form_of)           one set per reachable (form, residual type, relu) class of the fused entry points (int8 x), then
                                  the sets on the shy 0 | 1 edge for an int16 residual"""
import itertools

import topdown_nets

RANGE = range(-16, 17)
TYPE_PAIRS = ((1, 1), (1, 2), (2, 1), (2, 2))                       # (x_bytes, y_bytes)
FORMS = (0, 1, 2, 3)                                                # fp32, int32 k <= 0, int32 k > 0, packed int16
EDGES = {
    "g": (8, 9),
    "shx": (0, 1, 8, 9, 12, 13),
    "shy": (0, 1, 8, 9, 12, 13),
    "k": (-16, -15, 0, 1, 8, 9, 24, 25),
    "gx": (-16, 16), "gy": (-16, 16), "ib": (-16, 16),
}
# two ordinary settings: the ResNet tail (an int16 sum one grid finer than the conv result, packed form) and a coarse one with a
# left shift in the narrow output
ANCHORS = ({"g": 5, "shx": 1, "shy": 0, "k": 1}, {"g": 2, "shx": 0, "shy": 2, "k": -1})
# (ob3, g_res, ib) of tests/test_gpu_block_tail.py's CASES and (obp as g_res) PROJ_CASES; test_add_rule_cpu.py holds them together
BLOCK_TAIL_TRIPLES = ((4, 5, 4), (4, 4, 4), (3, 5, 4), (4, 5, 3), (5, 5, 5), (4, 6, 2), (3, 4, 4))


def quantities(gx, gy, ib):
    g = max(0, gx, gy)
    return {"g": g, "shx": g - gx, "shy": g - gy, "k": g - ib, "gx": gx, "gy": gy, "ib": ib}


def _all_sets():
    return [(gx, gy, ib) for gx in RANGE for gy in RANGE for ib in RANGE]


_EDGE_SETS = []


def edge_sets():
    """[(quantity, value, (gx, gy, ib))]: for every edge value, the nearest set to each anchor (distance: the sum of the absolute
    differences in the other selection quantities; ties by the order of _all_sets)."""
    if _EDGE_SETS:
        return list(_EDGE_SETS)
    sets = [(s, quantities(*s)) for s in _all_sets()]
    out = _EDGE_SETS
    for name, values in EDGES.items():
        for v in values:
            at = [(s, q) for s, q in sets if q[name] == v]
            assert at, (name, v)
            for anchor in ANCHORS:
                dist = lambda q: sum(abs(q[o] - anchor[o]) for o in anchor if o != name)
                out.append((name, v, min(at, key=lambda sq: dist(sq[1]))[0]))
    return list(out)


def project_sets():
    top = [(gx, gy, max(0, gx, gy) - k) for gx, gy in itertools.product(topdown_nets.GRIDS, repeat=2) for k in topdown_nets.K_VALUES]
    return list(BLOCK_TAIL_TRIPLES) + top


_TRIPLES = None


def triples():
    global _TRIPLES
    if _TRIPLES is None:
        seen, out = set(), []
        for s in [e[2] for e in edge_sets()] + project_sets():
            if s not in seen:
                seen.add(s)
                out.append(s)
        _TRIPLES = out
    return list(_TRIPLES)


def coverage(form_of):
    """{"forms": {(form, x_bytes, y_bytes, relu)}, "edges": {(quantity, value)}} of triples()."""
    forms = set()
    for (xb, yb) in TYPE_PAIRS:
        for relu in (0, 1):
            for (gx, gy, ib) in triples():
                forms.add((form_of(xb, gx, yb, gy, ib, relu), xb, yb, relu))
    edges = set()
    for s in triples():
        q = quantities(*s)
        edges |= {(name, q[name]) for name, values in EDGES.items() if q[name] in values}
    return {"forms": forms, "edges": edges}


def reachable_forms(xb, yb):
    """The forms an operand-type pair can take: the packed one needs an int8 x."""
    return FORMS if xb == 1 else FORMS[:3]


def class_sets(form_of, xb, yb):
    """[(gx, gy, ib, relu)]: for ReLU off and on and each form this operand-type pair can take, the first set of triples() that
    runs it with a wide output (g <= 8) -- and for the fp32 form, which is reached both by a shift beyond 12 and by g > 8, also
    the first set without one."""
    out = []
    for relu in (0, 1):
        for form in reachable_forms(xb, yb):
            hits = [s for s in triples() if form_of(xb, s[0], yb, s[1], s[2], relu) == form]
            assert hits, (xb, yb, relu, form)
            wide = [s for s in hits if quantities(*s)["g"] <= 8]
            out.append((wide or hits)[0] + (relu,))
            if form == 0 and wide and len(wide) < len(hits):
                out.append([s for s in hits if quantities(*s)["g"] > 8][0] + (relu,))
    return out


def fused_sets(form_of):
    """[(gx, gy, ib, y_bytes, relu)] for the fused entry points, whose x is a convolution's int8 result on the grid gx = ob:
    class_sets for an int8 and an int16 residual, then both sides of shy 0 | 1 with an int16 residual."""
    out = [s[:3] + (yb, s[3]) for yb in (1, 2) for s in class_sets(form_of, 1, yb)]
    for relu in (0, 1):
        for v in (0, 1):
            out += [s + (2, relu) for s in [e[2] for e in edge_sets() if e[:2] == ("shy", v)] if s + (2, relu) not in out]
    return out
