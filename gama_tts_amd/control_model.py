"""Compiles an articulatory database (a GamaTTS `artic.xml`) to the flat arrays of gvtm_rules_model (include/gama_vtm.h).

The reference keeps the database as objects: postures with categories, rules with one boolean expression tree per position,
equations as formula trees over 21 float symbols, transitions as lists of points and slope ratios.  What
EventList::generateEventList() asks of them is small, and every answer is a table:

  * does position k of rule r accept posture p, unmarked / marked          -> match[r][k][p], two bits
  * what is equation e on the current symbols                               -> a postfix program of float operations
  * which points does transition t have, in pointOrSlopeList() order        -> items over one pool of points and one of slopes

Nothing here computes an event; csrc/vtm_rules.hpp does, on the host and on the device, from these arrays alone.

The two grammars are restated from what the reference's parsers accept:

  boolean expression   node := NAME | "(" "marked" node ")" | "(" "not" node ")" | "(" node ("and" | "or" | "xor") node ")"
                       NAME is a posture's symbol (only that posture matches: its own category) or, failing that, a category.
                       Tokens end at white space and at parentheses only.
  formula              expression := term {("+" | "-") term};  term := factor {("*" | "/") factor}
                       factor := "(" expression ")" | "+" factor | "-" factor | SYMBOL | CONSTANT
                       A token that starts with none of + - * / ( ) runs to the next white space or parenthesis, so operators
                       must stand apart from names ("mark1 * 0.5"); a token that is no symbol must be a float constant.
"""
import fractions
import xml.etree.ElementTree as ET

import numpy as np

N_PARAM = 16
# FormulaSymbol::Code, in order
FORMULA_SYMBOLS = ("transition1", "transition2", "transition3", "transition4", "qssa1", "qssa2", "qssa3", "qssa4",
                   "qssb1", "qssb2", "qssb3", "qssb4", "tempo1", "tempo2", "tempo3", "tempo4", "rd", "beat", "mark1", "mark2", "mark3")
N_FORMULA_SYMBOLS = len(FORMULA_SYMBOLS)
SYM_RD, SYM_BEAT, SYM_MARK1, SYM_MARK2, SYM_MARK3 = 16, 17, 18, 19, 20
# the database's <symbols>, by position, that a posture's six symbol targets are (Posture::Symbol without the two durations)
POSTURE_SYMBOL_SLOTS = (1, 2, 3, 5, 6, 7)
N_POSTURE_SYMBOLS = 8
# program operations (gvtm_rules_model.program_op: the code in the low byte, a symbol's index above it)
OP_CONST, OP_SYMBOL, OP_NEG, OP_ADD, OP_SUB, OP_MUL, OP_DIV = range(7)
# rule_equations columns
EQ_DURATION, EQ_BEAT, EQ_MARK1, EQ_MARK2, EQ_MARK3 = range(5)
ITEM_POINT, ITEM_SLOPE_RATIO = 0, 1
POINT_TYPES = {"diphone": 2, "triphone": 3, "tetraphone": 4}

ARRAYS = ("param_target", "symbol_target", "param_min", "param_max", "rule_n_expr", "rule_equations", "rule_param_transition",
          "rule_special_transition", "match", "equation_offsets", "program_op", "program_const", "transition_offsets", "items",
          "point_type", "point_value", "point_free_time", "point_time_eq", "slopes")


class ModelError(ValueError):
    pass


def parse_float32(text):
    """A decimal string to the nearest float32, rounded once (through float64 it would be rounded twice)."""
    text = text.strip()
    try:
        near = np.float32(float(text))
    except ValueError:
        raise ModelError("not a number: %r" % text)
    if not np.isfinite(near):
        return near
    try:
        exact = fractions.Fraction(text)
    except ValueError:
        return near
    best = near
    for other in (np.nextafter(near, np.float32(-np.inf)), np.nextafter(near, np.float32(np.inf))):
        if not np.isfinite(other):
            continue
        d_best, d_other = abs(fractions.Fraction(float(best)) - exact), abs(fractions.Fraction(float(other)) - exact)
        if d_other < d_best or (d_other == d_best and (other.view(np.uint32) & 1) == 0 and (best.view(np.uint32) & 1) == 1):
            best = other
    return best


def _tokens(text, operators):
    """Tokens of either grammar: parentheses and `operators` are one character each where a token starts; anything else
    runs to the next white space or parenthesis."""
    out, i, n = [], 0, len(text)
    while i < n:
        c = text[i]
        if c.isspace():
            i += 1
        elif c in "()" or c in operators:
            out.append(c)
            i += 1
        else:
            j = i
            while j < n and not text[j].isspace() and text[j] not in "()":
                j += 1
            out.append(text[i:j])
            i = j
    return out


def compile_boolean(text, posture_ids, category_members, n_postures):
    """One position's expression -> uint8 [n_postures], bit 0: holds for the posture unmarked, bit 1: marked."""
    tokens = _tokens(text, "")
    if not tokens:
        raise ModelError("empty boolean expression")
    pos = 0

    def node():
        nonlocal pos
        if pos >= len(tokens):
            raise ModelError("boolean expression ends early: %r" % text)
        t = tokens[pos]
        pos += 1
        if t == "(":
            if pos >= len(tokens):
                raise ModelError("boolean expression ends early: %r" % text)
            if tokens[pos] == "marked":
                pos += 1
                a = node()
                r = (np.zeros_like(a[0]), a[1])
            elif tokens[pos] == "not":
                pos += 1
                a = node()
                r = (~a[0], ~a[1])
            else:
                a = node()
                op = tokens[pos] if pos < len(tokens) else None
                if op not in ("and", "or", "xor"):
                    raise ModelError("missing operator in %r" % text)
                pos += 1
                b = node()
                if op == "and":
                    r = (a[0] & b[0], a[1] & b[1])
                elif op == "or":
                    r = (a[0] | b[0], a[1] | b[1])
                else:
                    r = (a[0] ^ b[0], a[1] ^ b[1])
            if pos >= len(tokens) or tokens[pos] != ")":
                raise ModelError("right parenthesis not found in %r" % text)
            pos += 1
            return r
        if t in (")", "and", "or", "xor", "not"):
            raise ModelError("unexpected %r in %r" % (t, text))
        members = np.zeros(n_postures, dtype=bool)
        if t in posture_ids:  # a posture's own category: that posture alone
            members[posture_ids[t]] = True
        elif t in category_members:
            members[list(category_members[t])] = True
        else:
            raise ModelError("could not find category %r in %r" % (t, text))
        return members, members.copy()

    unmarked, marked = node()
    if pos != len(tokens):
        raise ModelError("text after the expression in %r" % text)
    return unmarked.astype(np.uint8) | (marked.astype(np.uint8) << 1)


def compile_formula(text):
    """A formula -> (ops int32 [n], constants float32 [n]), postfix."""
    tokens = _tokens(text, "+-*/")
    if not tokens:
        raise ModelError("empty formula")
    ops, consts = [], []
    pos = 0

    def emit(op, const=0.0):
        ops.append(op)
        consts.append(np.float32(const))

    def peek():
        return tokens[pos] if pos < len(tokens) else None

    def factor():
        nonlocal pos
        t = peek()
        if t is None:
            raise ModelError("formula ends early: %r" % text)
        pos += 1
        if t == "(":
            expression()
            if peek() != ")":
                raise ModelError("right parenthesis not found in %r" % text)
            pos += 1
        elif t == "+":
            factor()
        elif t == "-":
            factor()
            emit(OP_NEG)
        elif t in (")", "*", "/"):
            raise ModelError("unexpected %r in %r" % (t, text))
        elif t in FORMULA_SYMBOLS:
            emit(OP_SYMBOL | (FORMULA_SYMBOLS.index(t) << 8))
        else:
            emit(OP_CONST, parse_float32(t))

    def term():
        nonlocal pos
        factor()
        while peek() in ("*", "/"):
            op = tokens[pos]
            pos += 1
            factor()
            emit(OP_MUL if op == "*" else OP_DIV)

    def expression():
        nonlocal pos
        term()
        while peek() in ("+", "-"):
            op = tokens[pos]
            pos += 1
            term()
            emit(OP_ADD if op == "+" else OP_SUB)

    expression()
    if pos != len(tokens):
        raise ModelError("text after the formula in %r" % text)
    return np.asarray(ops, dtype=np.int32), np.asarray(consts, dtype=np.float32)


def evaluate_program(ops, consts, symbols):
    """Runs one postfix program on float32 symbols [21]: one float32 rounding per operation, as the rule does."""
    symbols = np.asarray(symbols, dtype=np.float32)
    stack = []
    with np.errstate(all="ignore"):
        for op, c in zip(ops, consts):
            code = int(op) & 0xFF
            if code == OP_CONST:
                stack.append(np.float32(c))
            elif code == OP_SYMBOL:
                stack.append(symbols[int(op) >> 8])
            elif code == OP_NEG:
                stack.append(np.float32(-stack.pop()))
            else:
                b, a = stack.pop(), stack.pop()
                stack.append(np.float32({OP_ADD: a + b, OP_SUB: a - b, OP_MUL: a * b, OP_DIV: np.divide(a, b)}[code]))
    assert len(stack) == 1
    return stack[0]


def evaluate_equation(model, equation, symbols):
    lo, hi = model["equation_offsets"][equation], model["equation_offsets"][equation + 1]
    return evaluate_program(model["program_op"][lo:hi], model["program_const"][lo:hi], symbols)


def _children(elem, tag):
    return [] if elem is None else [c for c in elem if c.tag == tag]


def _attr(elem, name, optional=False):
    v = elem.get(name)
    if v is None:
        if optional:
            return ""
        raise ModelError("<%s> without %s" % (elem.tag, name))
    return v


def compile_model(source):
    """`source`: the path of an artic.xml, or its text.  Returns a dict: the arrays named in ARRAYS (what gvtm_rules_model
    points at), vocoid (uint8 [postures], or None) and the name lists posture_names, equation_names, transition_names (numpy string arrays; ids are positions; the postures are in
    the reference's order, sorted by name)."""
    root = ET.fromstring(source) if source.lstrip().startswith("<") else ET.parse(source).getroot()
    categories = [_attr(c, "name") for c in _children(root.find("categories"), "category")]
    parameters = _children(root.find("parameters"), "parameter")
    if len(parameters) != N_PARAM:
        raise ModelError("%d parameters, not %d" % (len(parameters), N_PARAM))
    param_names = [_attr(p, "name") for p in parameters]
    param_index = {}
    for i, n in enumerate(param_names):
        param_index.setdefault(n, i)
    symbol_names = [_attr(s, "name") for s in _children(root.find("symbols"), "symbol")]
    if len(symbol_names) != N_POSTURE_SYMBOLS:
        raise ModelError("%d symbols, not %d" % (len(symbol_names), N_POSTURE_SYMBOLS))

    # (PostureList keeps its postures sorted by name, byte by byte, and takes no name twice: a posture's id is its place there)
    postures = sorted(_children(root.find("postures"), "posture"), key=lambda e: _attr(e, "symbol").encode())
    n_postures = len(postures)
    posture_names = [_attr(p, "symbol") for p in postures]
    if len(set(posture_names)) != n_postures:
        raise ModelError("duplicate posture name")
    posture_ids = {n: i for i, n in enumerate(posture_names)}
    category_members = {}
    for c in categories:
        category_members.setdefault(c, set())
    param_target = np.zeros((n_postures, N_PARAM), dtype=np.float32)
    all_symbols = np.zeros((n_postures, N_POSTURE_SYMBOLS), dtype=np.float32)
    for p, elem in enumerate(postures):
        for child in elem:
            if child.tag == "posture-categories":
                for ref in _children(child, "category-ref"):
                    name = _attr(ref, "name")
                    if name != posture_names[p]:
                        if name not in category_members:
                            raise ModelError("posture category not found: %r" % name)
                        category_members[name].add(p)
            elif child.tag == "parameter-targets":
                for t in _children(child, "target"):
                    name = _attr(t, "name")
                    if name not in param_index:
                        raise ModelError("parameter name not found: %r" % name)
                    param_target[p, param_index[name]] = parse_float32(_attr(t, "value"))
            elif child.tag == "symbol-targets":
                for t in _children(child, "target"):
                    value = parse_float32(_attr(t, "value"))
                    for i, n in enumerate(symbol_names):
                        if n == _attr(t, "name"):
                            all_symbols[p, i] = value

    # equations: one list over the groups; one without a formula is dropped, as the reference drops it
    equation_names, programs = [], []
    for group in _children(root.find("equations"), "equation-group"):
        for eq in _children(group, "equation"):
            formula = _attr(eq, "formula", optional=True)
            if formula.strip():
                equation_names.append(_attr(eq, "name"))
                programs.append(compile_formula(formula))
    equation_ids = {}
    for i, n in enumerate(equation_names):
        equation_ids.setdefault(n, i)

    def equation_id(name):
        if name not in equation_ids:
            raise ModelError("equation not found: %r" % name)
        return equation_ids[name]

    # transitions: the regular ones, then the special ones, in one list; a name is looked up within its kind
    transition_names, items_of = [], []
    point_type, point_value, point_free_time, point_time_eq, slopes = [], [], [], [], []

    def add_point(elem):
        kind = _attr(elem, "type")
        if kind not in POINT_TYPES:
            raise ModelError("invalid transition point type: %r" % kind)
        point_type.append(POINT_TYPES[kind])
        point_value.append(parse_float32(_attr(elem, "value")))
        time_expression = _attr(elem, "time-expression", optional=True)
        if time_expression:
            point_free_time.append(np.float32(0.0))
            point_time_eq.append(equation_id(time_expression))
        else:
            point_free_time.append(parse_float32(_attr(elem, "free-time")))
            point_time_eq.append(-1)

    def add_transitions(section):
        ids = {}
        for group in _children(root.find(section), "transition-group"):
            for tr in _children(group, "transition"):
                if _attr(tr, "type") not in POINT_TYPES:
                    raise ModelError("invalid transition type: %r" % _attr(tr, "type"))
                items = []
                for pos in _children(tr, "point-or-slopes"):
                    for child in pos:
                        if child.tag == "point":
                            items.append((ITEM_POINT, len(point_type), 1, len(slopes), 0))
                            add_point(child)
                        elif child.tag == "slope-ratio":
                            first_point, first_slope = len(point_type), len(slopes)
                            for part in child:
                                if part.tag == "points":
                                    for pt in _children(part, "point"):
                                        add_point(pt)
                            # (points of the <points> and slopes of the <slopes> elements each form one run)
                            for part in child:
                                if part.tag == "slopes":
                                    for s in _children(part, "slope"):
                                        slopes.append(parse_float32(_attr(s, "slope")))
                            items.append((ITEM_SLOPE_RATIO, first_point, len(point_type) - first_point, first_slope, len(slopes) - first_slope))
                ids.setdefault(_attr(tr, "name"), len(transition_names))
                transition_names.append(_attr(tr, "name"))
                items_of.append(items)
        return ids

    regular_ids = add_transitions("transitions")
    special_ids = add_transitions("special-transitions")

    rules = _children(root.find("rules"), "rule")
    n_rules = len(rules)
    rule_n_expr = np.zeros(n_rules, dtype=np.int32)
    rule_equations = np.full((n_rules, 5), -1, dtype=np.int32)
    rule_param = np.full((n_rules, N_PARAM), -1, dtype=np.int32)
    rule_special = np.full((n_rules, N_PARAM), -1, dtype=np.int32)
    match = np.zeros((n_rules, 4, n_postures), dtype=np.uint8)
    symbol_column = {"rd": EQ_DURATION, "beat": EQ_BEAT, "mark1": EQ_MARK1, "mark2": EQ_MARK2, "mark3": EQ_MARK3}
    for r, rule in enumerate(rules):
        for child in rule:
            if child.tag == "boolean-expressions":
                expressions = [e.text or "" for e in _children(child, "boolean-expression")]
                if not 2 <= len(expressions) <= 4:
                    raise ModelError("rule %d: %d boolean expressions" % (r + 1, len(expressions)))
                rule_n_expr[r] = len(expressions)
                for k, text in enumerate(expressions):
                    match[r, k] = compile_boolean(text, posture_ids, category_members, n_postures)
            elif child.tag in ("parameter-profiles", "special-profiles"):
                table, ids = (rule_param, regular_ids) if child.tag == "parameter-profiles" else (rule_special, special_ids)
                for pt in _children(child, "parameter-transition"):
                    name, transition = _attr(pt, "name"), _attr(pt, "transition")
                    if name not in param_index:
                        raise ModelError("parameter name not found: %r" % name)
                    if transition not in ids:
                        raise ModelError("transition not found: %r" % transition)
                    table[r, param_index[name]] = ids[transition]
            elif child.tag == "expression-symbols":
                for se in _children(child, "symbol-equation"):
                    eq = equation_id(_attr(se, "equation"))
                    if _attr(se, "name") in symbol_column:
                        rule_equations[r, symbol_column[_attr(se, "name")]] = eq
        if rule_n_expr[r] == 0:
            raise ModelError("rule %d has no boolean expressions" % (r + 1))

    def offsets(lengths):
        return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)

    return {
        "param_target": param_target,
        "symbol_target": np.ascontiguousarray(all_symbols[:, POSTURE_SYMBOL_SLOTS]),
        "param_min": np.asarray([parse_float32(_attr(p, "minimum")) for p in parameters], dtype=np.float32),
        "param_max": np.asarray([parse_float32(_attr(p, "maximum")) for p in parameters], dtype=np.float32),
        "rule_n_expr": rule_n_expr,
        "rule_equations": rule_equations,
        "rule_param_transition": rule_param,
        "rule_special_transition": rule_special,
        "match": match,
        "equation_offsets": offsets([len(p[0]) for p in programs]),
        "program_op": np.concatenate([p[0] for p in programs] + [np.zeros(0, dtype=np.int32)]).astype(np.int32),
        "program_const": np.concatenate([p[1] for p in programs] + [np.zeros(0, dtype=np.float32)]).astype(np.float32),
        "transition_offsets": offsets([len(i) for i in items_of]),
        "items": np.asarray([i for items in items_of for i in items], dtype=np.int32).reshape(-1, 5),
        "point_type": np.asarray(point_type, dtype=np.int32),
        "point_value": np.asarray(point_value, dtype=np.float32),
        "point_free_time": np.asarray(point_free_time, dtype=np.float32),
        "point_time_eq": np.asarray(point_time_eq, dtype=np.int32),
        "slopes": np.asarray(slopes, dtype=np.float32),
        # is the posture a member of the category "vocoid" (EventList::applyIntonation's search); None: the database has no
        # such category.  Not one of ARRAYS: it goes to gvtm_prosody_create, not into gvtm_rules_model
        "vocoid": (np.asarray([p in category_members["vocoid"] for p in range(n_postures)], dtype=np.uint8)
                   if "vocoid" in category_members else None),
        "posture_names": np.asarray(posture_names),
        "equation_names": np.asarray(equation_names),
        "transition_names": np.asarray(transition_names),
    }
