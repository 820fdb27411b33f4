"""Utility programs: a user's own composite utility U(theta, y) as a straight-line program the device interprets
(include/bocf_hip.h, "utility programs"; the kernels are csrc/util_prog.hip).

`trace(func, m, theta_dim)` calls the NumPy callable once with dtype=object arrays of symbolic nodes, so whatever arithmetic it
does -- np.dot, np.sum(..., axis=0), np.square, np.multiply, np.exp ..., **, abs, unary minus, .transpose(), np.squeeze -- is
recorded as a graph over the closed operation set OPS.  The gradient dU/dy is derived from that graph by reverse-mode
differentiation (the operation set is closed under it) and is ordinary output of a second section, so the device needs a forward
evaluator only.  Both sections share common subexpressions (nodes are hash-consed), are scheduled to keep few values alive and
get their value slots from a liveness-based allocator.  `Program.to_bytes()` is the blob of the C ABI; `Program.value` /
`Program.value_and_grad` interpret the ENCODED instructions with NumPy, in their order, vectorised over columns: the check of the
tracer on the CPU and the host func / dfunc of a program utility.

What cannot be traced: data-dependent control flow.  Truth-testing a node (`if y[0] > 0:`, np.maximum, np.where, np.max, sorting)
raises TraceError; `maximum(a, b)` / `minimum(a, b)` of this module and comparisons used as 0/1 factors (`(y > 0) * y`) are the
traceable forms.  Constants the callable closes over become literals of the program: trace again when they change.  Non-finite
values are the user's responsibility (a program computes what its arithmetic gives)."""
import struct

import numpy as np

OPS = ("ADD", "SUB", "MUL", "DIV", "NEG", "ABS", "SIGN", "SQRT", "EXP", "LOG", "SIN", "COS", "TANH", "POW", "MIN", "MAX", "GE")
OP = {name: i for i, name in enumerate(OPS)}
K_SLOT, K_INPUT, K_PARAM, K_CONST = 0, 1, 2, 3

# mirrors of include/bocf_hip.h (tests/test_utility_program_cpu.py compares them with the header)
MAGIC, VERSION, HEADER_WORDS = 0x47505542, 1, 32
MAX_INSTR, MAX_SLOTS, MAX_CONSTS, MAX_M = 1024, 64, 256, 16


class TraceError(TypeError):
    """The callable cannot be written as a straight-line program."""


class ProgramLimitError(ValueError):
    """The traced program exceeds a limit of include/bocf_hip.h (the message names it)."""


def _bits(v):
    return struct.pack("<d", v)


class _Graph(object):
    def __init__(self):
        self.nodes = []
        self.cons = {}

    def _new(self, key, **kw):
        n = self.cons.get(key)
        if n is None:
            n = Node(self, len(self.nodes), **kw)
            self.nodes.append(n)
            self.cons[key] = n
        return n

    def const(self, v):
        v = float(v)
        return self._new(("const", _bits(v)), op="const", value=v)

    def input(self, j):
        return self._new(("input", j), op="input", index=j)

    def param(self, k):
        return self._new(("param", k), op="param", index=k)

    def lift(self, x):
        if isinstance(x, Node):
            if x.g is not self:
                raise TraceError("a node of another trace leaked into this one")
            return x
        if isinstance(x, np.ndarray) and x.ndim == 0:
            x = x.item()
            if isinstance(x, Node):
                return x
        if isinstance(x, (bool, int, float, np.integer, np.floating, np.bool_)):
            return self.const(x)
        return None

    def make(self, op, a, b=None, simplify=True):
        """Node of `op` (hash-consed).  Constant operands are folded; x*1, 1*x, x+0, 0+x, x-0, x/1, -(-x), x**1, x**2 -> x*x and 0*x -> 0
        are simplified (the last one assumes finite x)."""
        if simplify:
            ca = a.value if a.op == "const" else None
            cb = b.value if (b is not None and b.op == "const") else None
            if ca is not None and (b is None or cb is not None):
                return self.const(_fold(op, ca, cb))
            if op == "MUL":
                if ca == 1.0:
                    return b
                if cb == 1.0:
                    return a
                if ca == 0.0 or cb == 0.0:
                    return self.const(0.0)
            elif op == "ADD":
                if ca == 0.0:
                    return b
                if cb == 0.0:
                    return a
            elif op == "SUB" and cb == 0.0:
                return a
            elif op == "DIV" and cb == 1.0:
                return a
            elif op == "NEG" and a.op == "NEG":
                return a.a
            elif op == "POW" and cb is not None:
                if cb == 1.0:
                    return a
                if cb == 2.0:
                    return self.make("MUL", a, a)
                if cb == 0.0:
                    return self.const(1.0)
        key = (op, a.id, -1 if b is None else b.id)
        return self._new(key, op=op, a=a, b=b)


def _fold(op, a, b):
    with np.errstate(all="ignore"):
        return float(_NP[OP[op]](np.float64(a), None if b is None else np.float64(b)))


class Node(object):
    """One value of the traced expression.  Arithmetic builds new nodes; a truth test raises TraceError."""
    __slots__ = ("g", "id", "op", "a", "b", "value", "index")

    def __init__(self, g, id, op, a=None, b=None, value=None, index=None):
        self.g, self.id, self.op, self.a, self.b, self.value, self.index = g, id, op, a, b, value, index

    def _bin(self, op, other, swap=False):
        o = self.g.lift(other)
        if o is None:
            return NotImplemented
        return self.g.make(op, o, self) if swap else self.g.make(op, self, o)

    def __add__(self, o): return self._bin("ADD", o)
    def __radd__(self, o): return self._bin("ADD", o, True)
    def __sub__(self, o): return self._bin("SUB", o)
    def __rsub__(self, o): return self._bin("SUB", o, True)
    def __mul__(self, o): return self._bin("MUL", o)
    def __rmul__(self, o): return self._bin("MUL", o, True)
    def __truediv__(self, o): return self._bin("DIV", o)
    def __rtruediv__(self, o): return self._bin("DIV", o, True)
    def __pow__(self, o): return self._bin("POW", o)
    def __rpow__(self, o): return self._bin("POW", o, True)
    def __neg__(self): return self.g.make("NEG", self)
    def __pos__(self): return self
    def __abs__(self): return self.g.make("ABS", self)

    # comparisons give 0/1 values (usable as factors); testing their truth is control flow
    def __ge__(self, o): return self._bin("GE", o)
    def __le__(self, o): return self._bin("GE", o, True)

    def __gt__(self, o):
        r = self._bin("GE", o, True)
        return r if r is NotImplemented else 1.0 - r

    def __lt__(self, o):
        r = self._bin("GE", o)
        return r if r is NotImplemented else 1.0 - r

    def __bool__(self):
        raise TraceError("the utility tests the truth of a value that depends on y or theta (if / while, np.maximum, np.where, np.max, "
                         "sorting ...): data-dependent control flow cannot be traced into a straight-line program; use "
                         "bocf_amd.utility_program.maximum / minimum or a comparison as a 0/1 factor")

    def __float__(self):
        raise TraceError("the utility converts a traced value to a Python float: it cannot be traced")

    __hash__ = object.__hash__

    def exp(self): return self.g.make("EXP", self)
    def log(self): return self.g.make("LOG", self)
    def sin(self): return self.g.make("SIN", self)
    def cos(self): return self.g.make("COS", self)
    def tanh(self): return self.g.make("TANH", self)
    def sqrt(self): return self.g.make("SQRT", self)
    def sign(self): return self.g.make("SIGN", self)
    def conjugate(self): return self

    def __repr__(self):
        if self.op == "const":
            return "%r" % self.value
        if self.op in ("input", "param"):
            return "%s%d" % ("y" if self.op == "input" else "theta", self.index)
        return "%s#%d" % (self.op, self.id)


def _has_node(x):
    if isinstance(x, Node):
        return True
    return isinstance(x, np.ndarray) and x.dtype == object


def _elementwise(op, ufunc, a, b):
    if not (_has_node(a) or _has_node(b)):
        return ufunc(a, b)

    def one(x, y):
        n = x if isinstance(x, Node) else y
        if not isinstance(n, Node):
            return float(ufunc(x, y))
        return n.g.make(op, n.g.lift(x), n.g.lift(y))
    return np.frompyfunc(one, 2, 1)(a, b)


def maximum(a, b):
    """Element-wise maximum that can be traced (np.maximum on traced values cannot)."""
    return _elementwise("MAX", np.maximum, a, b)


def minimum(a, b):
    """Element-wise minimum that can be traced."""
    return _elementwise("MIN", np.minimum, a, b)


# ---- reverse-mode differentiation ------------------------------------------------------------------------------------------------
def _reachable(roots):
    seen, stack = {}, list(roots)
    while stack:
        n = stack.pop()
        if n.id in seen:
            continue
        seen[n.id] = n
        if n.a is not None:
            stack.append(n.a)
        if n.b is not None:
            stack.append(n.b)
    return seen


def _gradient(g, root, m):
    """[dU/dy_0 ... dU/dy_{m-1}] as nodes of the same graph."""
    nodes = _reachable([root])
    adj = {root.id: g.const(1.0)}

    def add(n, v):
        if n.op in ("const", "param"):
            return
        adj[n.id] = v if n.id not in adj else g.make("ADD", adj[n.id], v)
    for i in sorted(nodes, reverse=True):             # operands are created before their results: decreasing id is reverse topological
        n = nodes[i]
        gr = adj.get(i)
        if gr is None or n.op in ("const", "param", "input"):
            continue
        a, b, op = n.a, n.b, n.op
        if op == "ADD":
            add(a, gr); add(b, gr)
        elif op == "SUB":
            add(a, gr); add(b, g.make("NEG", gr))
        elif op == "MUL":
            add(a, g.make("MUL", gr, b)); add(b, g.make("MUL", gr, a))
        elif op == "DIV":
            add(a, g.make("DIV", gr, b)); add(b, g.make("NEG", g.make("DIV", g.make("MUL", gr, n), b)))
        elif op == "NEG":
            add(a, g.make("NEG", gr))
        elif op == "ABS":
            add(a, g.make("MUL", gr, g.make("SIGN", a)))
        elif op == "SQRT":
            add(a, g.make("DIV", gr, g.make("MUL", g.const(2.0), n)))
        elif op == "EXP":
            add(a, g.make("MUL", gr, n))
        elif op == "LOG":
            add(a, g.make("DIV", gr, a))
        elif op == "SIN":
            add(a, g.make("MUL", gr, g.make("COS", a)))
        elif op == "COS":
            add(a, g.make("NEG", g.make("MUL", gr, g.make("SIN", a))))
        elif op == "TANH":
            add(a, g.make("MUL", gr, g.make("SUB", g.const(1.0), g.make("MUL", n, n))))
        elif op == "POW":
            if a.op not in ("const", "param"):
                add(a, g.make("MUL", gr, g.make("MUL", b, g.make("POW", a, g.make("SUB", b, g.const(1.0))))))
            if b.op not in ("const", "param"):
                add(b, g.make("MUL", gr, g.make("MUL", n, g.make("LOG", a))))
        elif op in ("MIN", "MAX"):                     # the operand that is taken gets the adjoint (a on ties)
            first = g.make("GE", b, a) if op == "MIN" else g.make("GE", a, b)
            add(a, g.make("MUL", gr, first)); add(b, g.make("MUL", gr, g.make("SUB", g.const(1.0), first)))
        # SIGN, GE: piecewise constant
    return [adj.get(g.input(j).id, g.const(0.0)) for j in range(m)]


# ---- scheduling, slot allocation, encoding ---------------------------------------------------------------------------------------
def _is_op(n):
    return n.op not in ("const", "input", "param")


def _dfs_order(outs):
    """Post-order from the outputs; the operand with the larger Sethi-Ullman label (slots its subtree needs) goes first."""
    reach = _reachable(outs)
    need = {}
    for i in sorted(reach):                            # ids are topological: operands are created before their results
        n = reach[i]
        if not _is_op(n):
            continue
        lab = sorted((need[k.id] for k in (n.a, n.b) if k is not None and _is_op(k)), reverse=True)
        need[i] = 1 if not lab else (lab[0] if len(lab) == 1 or lab[0] != lab[1] else lab[0] + 1)
    order, done = [], set()
    for root in outs:
        stack = [(root, False)]
        while stack:
            n, emit = stack.pop()
            if n.id in done:
                continue
            if emit:
                done.add(n.id)
                order.append(n)
                continue
            stack.append((n, True))
            kids = sorted((k for k in (n.a, n.b) if k is not None and _is_op(k)), key=lambda k: -need[k.id])
            for k in reversed(kids):
                stack.append((k, False))
    return order


def _greedy_order(outs, base):
    """List schedule: of the instructions whose operands are there, the one that lets most values die goes next (ties: the order of
    `base`).  A gradient shares its forward values with U; this interleaves the two so that they are not all alive at once."""
    pos = {n.id: t for t, n in enumerate(base)}
    kids = {n.id: list({k.id: k for k in (n.a, n.b) if k is not None and _is_op(k)}.values()) for n in base}
    uses = {n.id: 0 for n in base}
    for n in base:
        for k in kids[n.id]:
            uses[k.id] += 1
    for o in outs:
        uses[o.id] += 1                                # an output never dies
    waiting = {n.id: len(kids[n.id]) for n in base}
    users = {n.id: [] for n in base}
    for n in base:
        for k in kids[n.id]:
            users[k.id].append(n)
    ready = [n for n in base if waiting[n.id] == 0]
    order = []
    while ready:
        best = max(ready, key=lambda n: (sum(1 for k in kids[n.id] if uses[k.id] == 1), -pos[n.id]))
        ready.remove(best)
        order.append(best)
        for k in kids[best.id]:
            uses[k.id] -= 1
        for u in users[best.id]:
            waiting[u.id] -= 1
            if waiting[u.id] == 0:
                ready.append(u)
    return order


def _allocate(order, outs, consts):
    """Slots by liveness: a value's slot is free again after the last instruction that reads it (outputs stay to the end)."""
    last = {}
    for t, n in enumerate(order):
        for k in (n.a, n.b):
            if k is not None and _is_op(k):
                last[k.id] = t
    for o in outs:
        last[o.id] = len(order)
    free, slot, used = [], {}, 0
    code = []

    def operand(k):
        if k.op == "input":
            return K_INPUT << 14 | k.index
        if k.op == "param":
            return K_PARAM << 14 | k.index
        if k.op == "const":
            key = _bits(k.value)
            if key not in consts:
                consts[key] = len(consts)
            return K_CONST << 14 | consts[key]
        return K_SLOT << 14 | slot[k.id]
    for t, n in enumerate(order):
        a = operand(n.a)
        b = a if n.b is None else operand(n.b)
        for k in {k.id: k for k in (n.a, n.b) if k is not None and _is_op(k)}.values():
            if last[k.id] == t:                        # both operands are read before the destination is written: the slot is free again
                free.append(slot[k.id])
        if free:
            s = min(free)
            free.remove(s)
        else:
            s = used
            used += 1
        slot[n.id] = s
        code.append((OP[n.op], s, a, b))
    return code, [slot[o.id] for o in outs], used


def _section(g, outputs, consts):
    """(instructions [(opcode, dst slot, operand a, operand b)], output slots, slots used) for the output nodes: the schedule that
    needs fewer slots of the depth-first and the greedy one."""
    one = g.const(1.0)
    outs = [o if _is_op(o) else g.make("MUL", o, one, simplify=False) for o in outputs]      # an output lives in a slot
    base = _dfs_order(outs)
    best = None
    for order in (base, _greedy_order(outs, base)):
        trial = dict(consts)
        got = _allocate(order, outs, trial)
        if best is None or got[2] < best[0][2]:
            best = (got, trial)
    consts.update(best[1])
    return best[0]


class Program(object):
    """A traced utility: two instruction sections over `n_slots` value slots and a constant pool (layout: include/bocf_hip.h)."""

    def __init__(self, m, theta_dim, n_slots, val_code, val_out, grad_code, grad_outs, consts):
        self.m, self.theta_dim, self.n_slots = int(m), int(theta_dim), int(n_slots)
        self.val_code, self.val_out = list(val_code), int(val_out)
        self.grad_code, self.grad_outs = list(grad_code), [int(s) for s in grad_outs]
        self.consts = np.asarray(consts, dtype=np.float64).reshape(-1)

    def check_limits(self):
        for what, have, lim in (("BOCF_PROG_MAX_INSTR (instructions of the value section)", len(self.val_code), MAX_INSTR),
                                ("BOCF_PROG_MAX_INSTR (instructions of the value+gradient section)", len(self.grad_code), MAX_INSTR),
                                ("BOCF_PROG_MAX_SLOTS (values alive at once)", self.n_slots, MAX_SLOTS),
                                ("BOCF_PROG_MAX_CONSTS (constants)", self.consts.size, MAX_CONSTS),
                                ("BOCF_MAX_M (outputs)", self.m, MAX_M)):
            if have > lim:
                raise ProgramLimitError("the utility program exceeds %s: %d > %d" % (what, have, lim))
        return self

    def to_bytes(self):
        head = [MAGIC, VERSION, self.m, self.theta_dim, self.n_slots, len(self.val_code), len(self.grad_code), self.consts.size, self.val_out]
        head += self.grad_outs
        head += [0] * (HEADER_WORDS - len(head))
        words = []
        for op, dst, a, b in self.val_code + self.grad_code:
            words += [op | dst << 8, a | b << 16]
        return struct.pack("<%dI" % (HEADER_WORDS + len(words)), *(head + words)) + self.consts.astype("<f8").tobytes()

    @classmethod
    def from_bytes(cls, blob):
        blob = bytes(blob)
        if len(blob) < 4 * HEADER_WORDS:
            raise ValueError("utility program: truncated blob")
        head = struct.unpack_from("<%dI" % HEADER_WORDS, blob)
        if head[0] != MAGIC or head[1] != VERSION:
            raise ValueError("utility program: wrong magic / version")
        m, theta_dim, n_slots, nv, ng, nc, val_out = head[2:9]
        if m > MAX_M or len(blob) != 4 * HEADER_WORDS + 8 * (nv + ng + nc):
            raise ValueError("utility program: the blob's size does not match its header")
        w = struct.unpack_from("<%dI" % (2 * (nv + ng)), blob, 4 * HEADER_WORDS)
        code = [(w[2 * i] & 0xff, w[2 * i] >> 8, w[2 * i + 1] & 0xffff, w[2 * i + 1] >> 16) for i in range(nv + ng)]
        consts = np.frombuffer(blob, dtype="<f8", count=nc, offset=4 * HEADER_WORDS + 8 * (nv + ng))
        return cls(m, theta_dim, n_slots, code[:nv], val_out, code[nv:], head[9:10 + m], consts)

    # ---- the NumPy interpreter: the encoded instructions, in their order, one column per sample
    def _run(self, code, outs, theta, y):
        y = np.asarray(y, dtype=np.float64)
        single = y.ndim == 1
        Y = y.reshape(self.m, -1)
        theta = np.asarray(theta, dtype=np.float64).reshape(-1)
        if theta.size < self.theta_dim:
            raise ValueError("the utility program reads %d parameters, theta has %d" % (self.theta_dim, theta.size))
        f = np.empty((self.m + self.n_slots, Y.shape[1]))
        f[:self.m] = Y
        m, consts = self.m, self.consts

        def operand(o):
            kind, idx = o >> 14, o & 0x3fff
            if kind == K_SLOT:
                return f[m + idx]
            if kind == K_INPUT:
                return f[idx]
            return theta[idx] if kind == K_PARAM else consts[idx]
        with np.errstate(all="ignore"):
            for op, dst, a, b in code:
                f[m + dst] = _NP[op](operand(a), operand(b))
        out = f[[m + s for s in outs]]
        return out[:, 0] if single else out

    def value(self, theta, y):
        """U(theta, y): y (m,) -> float, y (m, n) -> (n,)."""
        r = self._run(self.val_code, [self.val_out], theta, y)[0]
        return float(r) if r.ndim == 0 else r

    def value_and_grad(self, theta, y):
        """(U, dU/dy): y (m,) -> (float, (m,)), y (m, n) -> ((n,), (m, n))."""
        r = self._run(self.grad_code, self.grad_outs, theta, y)
        return (float(r[0]) if r[0].ndim == 0 else r[0]), r[1:]

    def grad(self, theta, y):
        return self.value_and_grad(theta, y)[1]


_NP = [
    lambda a, b: a + b, lambda a, b: a - b, lambda a, b: a * b, lambda a, b: a / b, lambda a, b: -a, lambda a, b: np.abs(a),
    lambda a, b: np.sign(a), lambda a, b: np.sqrt(a), lambda a, b: np.exp(a), lambda a, b: np.log(a), lambda a, b: np.sin(a),
    lambda a, b: np.cos(a), lambda a, b: np.tanh(a), lambda a, b: np.power(a, b), lambda a, b: np.minimum(a, b),
    lambda a, b: np.maximum(a, b), lambda a, b: np.where(a >= b, 1.0, 0.0),
]


def trace(func, m, theta_dim):
    """Trace func(theta, y) -- theta (theta_dim,), y (m,), both dtype=object arrays of nodes -- into a Program (value section and
    value+gradient section).  Raises TraceError when the callable cannot be traced, ProgramLimitError when the program is too large."""
    m, theta_dim = int(m), int(theta_dim)
    if not 1 <= m <= MAX_M:
        raise ProgramLimitError("the utility program exceeds BOCF_MAX_M (outputs): m = %d, 1 .. %d" % (m, MAX_M))
    if not 0 <= theta_dim < (1 << 14):
        raise ValueError("theta_dim out of range")
    g = _Graph()
    theta, y = np.empty(theta_dim, dtype=object), np.empty(m, dtype=object)
    for k in range(theta_dim):
        theta[k] = g.param(k)
    for j in range(m):
        y[j] = g.input(j)
    try:
        out = func(theta, y)
    except TraceError:
        raise
    except Exception as e:
        raise TraceError("the utility could not be traced with symbolic arguments: %s: %s" % (type(e).__name__, e))
    flat = np.asarray(out, dtype=object).reshape(-1)
    if flat.size != 1:
        raise TraceError("the utility must return one value for y of shape (m,), it returned %d" % flat.size)
    root = g.lift(flat[0])
    if root is None:
        raise TraceError("the utility returned %r, not a number" % (type(flat[0]).__name__,))
    grads = _gradient(g, root, m)
    consts = {}
    val_code, val_out, s1 = _section(g, [root], consts)
    grad_code, grad_outs, s2 = _section(g, [root] + grads, consts)
    pool = np.array([struct.unpack("<d", k)[0] for k in sorted(consts, key=consts.get)], dtype=np.float64)
    return Program(m, theta_dim, max(s1, s2, 1), val_code, val_out[0], grad_code, grad_outs, pool).check_limits()
