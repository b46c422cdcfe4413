"""Wave-composition zoo: scenarios, labels and a dispatch predictor for the step kernel's velocity families.
TEST INFRASTRUCTURE ONLY -- the product package never loads it.

hk_velocity.h picks the velocity loop of a 64-lane wave from what ALL its running lanes hold (velocity_iterations,
vtwo_family, vone_family: about 25 template instantiations, re-picked at every chunk boundary).  The host build of
that source runs one lane at a time and cannot reach the mixed-wave paths, so the GPU tests have to -- with the
mix under control.  This module provides

  * the island probe (tests/native/island_probe.c, the oracle with a recorder on every island solve) and the
    labels it yields: per arena and step the island shapes, each island's period-4 exit iteration `cur`, the total
    island contacts and the TOI mini-island counts;
  * the seeded harvest of tests/golden/wave_zoo.npz (python tests/wave_zoo.py --harvest): one-arena scenarios
    (state, aux, K joint actions) whose REPLAY from set_state shows a wanted label;
  * a pure-Python restatement of the dispatch conditions (predict): the arms and events a wave must run;
  * the composition table (TABLE): which scenario class sits in which lane of which wave, and what each wave is for.

Shape keys: one bracket per island (solve order = the kernel's slot order), one `<A><B>p<points>` per contact,
`s` for a static body A, dynamic bodies numbered per island in first-appearance order.  `[01p1 s0p1]` is the S2
shape (player-puck, wall-player), `[s0p1 10p1]` a TB lane, `[s0p1 10p1 s1p1]` S3, `[s0p1][s0p1]` a SEP lane.
Length letters, one per island: S (cur <= 24), L (cur >= 100), M (between).  A class is `shape|letters`.
"""
import ctypes
import io
import os
import re
import subprocess
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")
PROBE_SRC = os.path.join(ROOT, "tests", "native", "island_probe.c")
PROBE_LIB = os.path.join(ORACLE_DIR, "libhk_island_probe.so")
FIXTURE = os.path.join(ROOT, "tests", "golden", "wave_zoo.npz")
if ORACLE_DIR not in sys.path:
    sys.path.insert(0, ORACLE_DIR)

K = 4  # steps per scenario
J = 1  # the label step of the composition table's rows (contacts persistent and warm-started); a few rows use 0
SHORT, LONG = 24, 100
CHUNK_STARTS = (0, 8, 16, 24, 56, 88, 120, 152)
VEL_ITERS = 180

# probe record layout (island_probe.c HKP_*)
_HEAD, _SOLVE, _MAXSOLVE = 6, 18, 4
REC = _HEAD + _MAXSOLVE * _SOLVE


# ------------------------------------------------------------------------------------------------ the probe
def build_probe():
    """Compile the probe next to the oracle library with the oracle Makefile's flags; returns its path."""
    srcs = [PROBE_SRC, os.path.join(ORACLE_DIR, "hk_oracle.c"), os.path.join(ORACLE_DIR, "hk_oracle.h")]
    if os.path.exists(PROBE_LIB) and os.path.getmtime(PROBE_LIB) >= max(os.path.getmtime(s) for s in srcs):
        return PROBE_LIB
    mk = open(os.path.join(ORACLE_DIR, "Makefile")).read()
    cflags = re.search(r"^CFLAGS\s*=\s*(.*)$", mk, re.M).group(1).split()
    tmp = PROBE_LIB + ".%d.tmp" % os.getpid()
    subprocess.check_call([os.environ.get("CC", "gcc"), *cflags, "-shared", "-o", tmp, PROBE_SRC, "-lm"])
    os.replace(tmp, PROBE_LIB)
    return PROBE_LIB


_probe = None


def probe_lib():
    global _probe
    if _probe is None:
        L = ctypes.CDLL(build_probe())
        vp = ctypes.c_void_p
        L.hkov_create.restype = vp
        L.hkov_create.argtypes = [ctypes.c_int64, vp, ctypes.c_uint64, ctypes.c_int64]
        L.hkov_destroy.argtypes = [vp]
        L.hkov_step.argtypes = [vp] * 13
        L.hkov_get_state.argtypes = [vp, vp, vp]
        L.hkov_set_state.argtypes = [vp, vp, vp, vp]
        L.hkp_arm.argtypes = [vp, ctypes.c_int64]
        L.hkp_rec_words.restype = ctypes.c_int
        assert L.hkp_rec_words() == REC
        _probe = L
    return _probe


def _vec_on(L, n, policies, auto_reset, seed=0):
    """An oracle.OracleVec bound to library L (the probe build exports the oracle's own hkov_* calls)."""
    import oracle as O

    v = O.OracleVec.__new__(O.OracleVec)
    v._L, v.n = L, int(n)
    cfg = np.array([1, 0, int(auto_reset), 0, O.POLICY[policies[0]], O.POLICY[policies[1]]], np.int32)
    v._v = L.hkov_create(v.n, cfg.ctypes.data, int(seed), 0)
    return v


def probe_replay(state, aux, actions):
    """Replay scenarios (state [n,18], aux [n,5], actions [K,n,8]) from set_state with external policies and no
    auto-reset, the probe armed.  Returns (records [K,n,REC] int32, ok [n]: finite and not done through K steps)."""
    L = probe_lib()
    n = state.shape[0]
    v = _vec_on(L, n, ("external", "external"), False)
    v.set_state(state, aux)
    rec = np.zeros((actions.shape[0], n, REC), np.int32)
    ok = np.ones(n, bool)
    try:
        for t in range(actions.shape[0]):
            L.hkp_arm(rec[t].ctypes.data, n)
            out = v.step(actions[t], with_agent_two=True)
            L.hkp_disarm()
            ok &= (out["done"] == 0) & np.isfinite(out["obs"]).all(1) & np.isfinite(out["obs2"]).all(1)
    finally:
        L.hkp_disarm()
        v.close()
    return rec, ok


# ------------------------------------------------------------------------------------------------ labels
LABEL_FIELDS = ("shape", "cur", "ncont", "toi", "toi_max", "toi_n2", "toi_big")


def shape_of(r):
    """Shape key and per-island cur ([4], 0 where no island) of one probe record."""
    out, cur = [], np.zeros(_MAXSOLVE, np.int16)
    for k in range(min(int(r[0]), _MAXSOLVE)):
        s = r[_HEAD + k * _SOLVE:_HEAD + (k + 1) * _SOLVE]
        n, cur[k] = int(s[0]), s[1]
        num, parts = {}, []
        for i in range(min(n, 4)):
            ia, ib, dyn, pts = (int(x) for x in s[2 + 4 * i:6 + 4 * i])
            a = "s"
            if dyn:
                a = str(num.setdefault(ia, len(num)))
            b = str(num.setdefault(ib, len(num)))
            parts.append("%s%sp%d" % (a, b, pts))
        if n > 4:
            parts.append("+%d" % (n - 4))
        out.append("[" + " ".join(parts) + "]")
    return "".join(out), cur


def labels_of(rec):
    """Probe records [K,n,REC] -> dict of label arrays, each [n,K,...] (the fixture's layout)."""
    k, n = rec.shape[:2]
    lab = {"shape": np.zeros((n, k), "S48"), "cur": np.zeros((n, k, _MAXSOLVE), np.int16)}
    for t in range(k):
        for i in range(n):
            if rec[t, i, 0]:
                s, c = shape_of(rec[t, i])
                assert len(s) <= 48, s
                lab["shape"][i, t], lab["cur"][i, t] = s.encode(), c
    for j, f in enumerate(("ncont", "toi", "toi_max", "toi_n2", "toi_big")):
        lab[f] = np.ascontiguousarray(rec[:, :, 1 + j].T.astype(np.int16))
    return lab


def letters(cur):
    return "".join("S" if c <= SHORT else ("L" if c >= LONG else "M") for c in cur if c > 0)


def class_of(shape, cur, toi=0):
    """`idle`: no island contact and no TOI event at the step."""
    shape = shape.decode() if isinstance(shape, bytes) else shape
    return "%s|%s" % (shape, letters(cur)) if shape else ("idle+toi" if toi else "idle")


DYNRIDER = "dynrider"


def is_dynrider(cls, shape):
    """A player-puck island that runs long beside the other player's short wall contact, that contact touching
    from the step before J to the step after: once it has retired, its impulses (saved and restored by the chunks
    the lane rides) are the next step's warm start."""
    return cls[J] in ("[01p1][s0p1]|LS", "[01p1][s0p2]|LS") and shape[J - 1] == shape[J] == shape[J + 1]


class Zoo:
    """The committed fixture: scenarios with their per-step labels, and the class -> scenario ids index."""

    def __init__(self, path=FIXTURE):
        with np.load(path, allow_pickle=False) as z:
            self.d = {k: z[k] for k in z.files}
        d = self.d
        self.n = d["state"].shape[0]
        self.cls = [[class_of(d["shape"][i, t], d["cur"][i, t], d["toi"][i, t]) for t in range(K)]
                    for i in range(self.n)]
        self.pool = {}  # (step, class) -> scenario ids, fixture order
        for i in range(self.n):
            for t in range(K):
                self.pool.setdefault((t, self.cls[i][t]), []).append(i)
        for i in range(self.n):  # TOI pools: by event count at the step, and lanes with a 2-contact mini-island
            for t in range(K):
                if d["toi"][i, t]:
                    self.pool.setdefault((t, "toi%d" % min(int(d["toi"][i, t]), 3)), []).append(i)
                if d["toi_n2"][i, t]:
                    self.pool.setdefault((t, "toim2"), []).append(i)
                if d["ncont"][i, t] > 4 and "M" not in self.cls[i][t].split("|")[-1]:
                    self.pool.setdefault((t, BIG), []).append(i)
            if is_dynrider(self.cls[i], d["shape"][i]):
                self.pool.setdefault((J, DYNRIDER), []).append(i)

    def lane(self, i, t):
        """(shape key, cur list) of scenario i at step t: the predictor's input for one lane."""
        return self.d["shape"][i, t].decode(), [int(c) for c in self.d["cur"][i, t] if c > 0]


# ------------------------------------------------------------------------------------------------ the predictor
class MidCur(Exception):
    """A wave holds an island with SHORT < cur < LONG: the two-checkpoint prediction is not sound for it."""


ARMS = ("vone<true,1>", "vone<true,2>", "vone<true,0>", "vone<false,1>", "vone<false,2>", "vone<false,0>",
        "vtwo<1,1,false>", "vtwo<1,2,false>", "vtwo<2,1,false>", "vtwo<2,2,false>", "vtwo<0,0,false>",
        "vtwo<0,0,true>", "s2<1,1>", "s2<0,1>", "s2<1,2>", "s2<0,2>", "alias<1,1>", "alias<1,0>", "alias<0,1>",
        "alias<0,0>", "s3<1,1>", "s3<0,0>", "vgen<reg,1>", "vgen<reg,0>", "hbm")
EVENTS = ("shift:s3->two", "shift:gen->two", "shift:two->one", "retire", "swap", "rider_retired_slot1",
          "rider_dyn_retired_slot1", "s3_rider", "s3_s2l")
# arms no lane mix of this scene reaches, each with the reason from the scene's geometry (at most 4 entries)
UNREACHABLE = {
    "vone<false,2>": "body A is dynamic only in player-puck contacts; those are polygon-circle contacts: one point",
}


def _slots(shape):
    """Contacts in slot order: (island, body A or None if static, body B, points); None for a lane whose island
    contacts are not all described (an island of more than 4 contacts)."""
    out = []
    for k, isl in enumerate(re.findall(r"\[([^\]]*)\]", shape)):
        for c in isl.split():
            if c.startswith("+"):
                return None
            m = re.fullmatch(r"(s|\d)(\d)p(\d)", c)
            out.append((k, None if m.group(1) == "s" else (k, int(m.group(1))), (k, int(m.group(2))), int(m.group(3))))
    return out


class _Lane:
    def __init__(self, shape, cur):
        self.slots = _slots(shape)
        self.cur = list(cur)
        self.retire = list(cur)  # per island: the iteration at which it leaves the loops
        self.hbm = self.slots is None or len(self.slots) > 4

    def live(self, it):
        return [i for i, s in enumerate(self.slots) if self.retire[s[0]] > it]

    def restart(self, it):  # a family switch restarts the snapshot chain: the next exit is at it + 8 at the earliest
        self.retire = [max(r, it + 8) if r > it else r for r in self.retire]


def _chunk_end(it):
    return min(it + (8 if it < 24 else 32), VEL_ITERS)


def _is_s3(sl):
    (_, a0, b0, p0), (_, a1, b1, p1), (_, a2, b2, p2) = sl
    return a0 is None and a2 is None and a1 is not None and b0 == b1 and a1 == b2 and p0 == p1 == p2 == 1


def _is_s2(c0, c1):
    return c1[1] is None and c1[2] == c0[1] and c0[0] == c1[0]


def predict(lanes, strict=True):
    """The dispatch of one wave at one step.  lanes: (shape key, cur list) per lane (idle lanes: ("", [])).

    Restates velocity_iterations / vtwo_family / vone_family of hk_velocity.h over the lanes' live contacts.  An
    island leaves the loops at its `cur` (exit needs the period-4 snapshot match) -- or, where a family switch at
    iteration b restarted the snapshot chain, at max(cur, b + 8); switches happen at chunk boundaries only, so an
    island with cur <= 24 has left by iteration 32 and one with cur >= 100 runs the chunk that starts at 56
    whatever happened before.  With strict, a wave holding an island in between is refused (MidCur), and the
    result is read at two checkpoints: `first` (iteration 0: a pure function of shapes and point counts) and
    `tail` (the chunk starting at 56; None if nothing runs then).  Returns {"first", "tail", "arms": {first, tail},
    "events", "trace": {chunk start: arm}}.  Lanes with more than 4 island contacts run the HBM slot file in a
    pass of their own ("hbm")."""
    L = [_Lane(s, c) for s, c in lanes if s]
    if strict and any(SHORT < c < LONG for l in L for c in l.cur):
        raise MidCur([l.cur for l in L])
    trace, events = {}, set()
    hbm = [l for l in L if l.hbm]
    for l in hbm:  # vgen_family<HbmSlots> without `leave`: islands retire at their cur
        ends = sorted(set(l.cur))
        if len(ends) > 1:
            events.add("retire")
    L = [l for l in L if not l.hbm]
    it, prev = 0, None

    def act(it):
        return [l for l in L if l.live(it)]

    while it < VEL_ITERS and act(it):
        A = act(it)
        nl = {id(l): len(l.live(it)) for l in A}
        s3 = [l for l in A if nl[id(l)] == 3 and l.live(it) == [0, 1, 2] and _is_s3(l.slots[:3])]
        s2l = [l for l in A if s3 and nl[id(l)] == 2 and _is_s2(*(l.slots[i] for i in l.live(it)))]
        if s3 and all(l in s3 or l in s2l or nl[id(l)] == 1 for l in A):
            fam = "s3"
        elif any(nl[id(l)] > 2 for l in A):
            fam = "gen"
        else:
            fam = "two" if any(nl[id(l)] > 1 for l in A) else "one"
        if prev is not None:
            events.add("shift:%s->%s" % (prev, fam))
            for l in A:
                l.restart(it)
        prev = fam
        if fam == "s3":
            one = True
            for l in A:
                lv = [l.slots[i] for i in l.live(it)]
                one = one and lv[0][3] == 1 and (l not in s2l or lv[1][3] == 1)
            if any(l not in s3 and l not in s2l for l in A):
                events.add("s3_rider")
            if s2l:
                events.add("s3_s2l")
            events.add("s3_entry")
            # the S3 family can only be entered at iteration 0 (a later dispatch follows a family that ends with at
            # most two live contacts per lane), where every lane's live contacts already sit in slots 0..n-1
            assert it == 0
            while it < VEL_ITERS and any(l.live(it) for l in s3):
                trace[it] = "s3<1,1>" if one else "s3<0,0>"
                it = _chunk_end(it)
        elif fam == "gen":
            p1 = all(l.slots[i][3] == 1 for l in A for i in l.live(it))
            while it < VEL_ITERS and any(len(l.live(it)) > 2 for l in L):
                trace[it] = "vgen<reg,1>" if p1 else "vgen<reg,0>"
                end = _chunk_end(it)
                for l in act(it):
                    n0 = len(l.live(it))
                    if any(0 < len(l.live(t)) < n0 for t in range(it + 4, end + 1, 4)):
                        events.add("retire")
                it = end
        else:
            ent = {}  # per lane: the contacts in slots 0 / 1 after the swap, fixed for the family
            for l in A:
                lv = l.live(it)
                if lv[0] != 0 or (fam == "two" and len(lv) > 1 and lv[1] != 1):
                    events.add("swap")
                ent[id(l)] = lv
            if fam == "one":
                while it < VEL_ITERS and act(it):
                    R = [l.slots[ent[id(l)][0]] for l in act(it)]
                    sa = all(c[1] is None for c in R)
                    p = 1 if all(c[3] == 1 for c in R) else (2 if all(c[3] == 2 for c in R) else 0)
                    trace[it] = "vone<%s,%d>" % ("true" if sa else "false", p)
                    it = _chunk_end(it)
            else:
                def st(l, it):
                    lv = ent[id(l)]
                    c0 = l.slots[lv[0]]
                    two = len(lv) > 1
                    c1 = l.slots[lv[1]] if two else None
                    sep = two and c0[0] != c1[0]
                    on0 = l.retire[c0[0]] > it
                    on1 = two and l.retire[c1[0]] > it
                    return dict(two=two, sep=sep, on0=on0, on1=on1, vc0=c0[3], vc1=c1[3] if two else 1, dyn0=c0[1],
                                s2=two and not sep and _is_s2(c0, c1), tb=two and not sep and c1[2] == c0[2],
                                nc=len(l.slots))

                while it < VEL_ITERS:
                    S = [st(l, it) for l in A]
                    S = [s for s in S if s["on0"] or s["on1"]]
                    if not S or not any(s["on0"] and s["on1"] for s in S):
                        break
                    two = [s for s in S if s["two"]]
                    s2ok = all(s["on0"] and (not s["two"] or (s["s2"] and s["on1"])) for s in S)
                    alok = all(s["on0"] and (not s["two"] or ((s["s2"] or s["tb"]) and s["on1"])) for s in S)
                    p0 = all(s["vc0"] == 1 for s in S)
                    if s2ok and all(s["vc1"] == 1 for s in two):
                        arm = "s2<%d,1>" % p0
                    elif s2ok and all(s["vc1"] == 2 for s in two):
                        arm = "s2<%d,2>" % p0
                    elif alok:
                        arm = "alias<%d,%d>" % (p0, all(s["vc1"] == 1 for s in two))
                    elif any(not s["on0"] for s in S):
                        arm = "vtwo<0,0,true>"
                    else:
                        arm = "vtwo<0,0,false>"
                        for a, b in ((1, 1), (1, 2), (2, 1), (2, 2)):
                            if all(s["vc0"] == a and (s["vc1"] == b if s["two"] or b == 1 else True) for s in S):
                                arm = "vtwo<%d,%d,false>" % (a, b)
                                break
                    trace[it] = arm
                    if arm[0] in "sa":
                        events.add("s2_chunk")
                        if any(not s["two"] and s["nc"] > 1 for s in S):
                            events.add("rider_retired_slot1")
                        if any(not s["two"] and s["nc"] > 1 and s["dyn0"] is not None for s in S):
                            events.add("rider_dyn_retired_slot1")
                    end = _chunk_end(it)
                    for l in A:
                        for t in range(it + 4, end + 1, 4):
                            s = st(l, t)
                            if s["sep"] and s["on0"] != s["on1"] and arm.startswith("vtwo"):
                                events.add("retire")
                    it = end
    first, tail = trace.get(0), trace.get(56)
    if hbm:
        trace["hbm"] = "hbm"
    return {"first": first, "tail": tail, "arms": {a for a in (first, tail, trace.get("hbm")) if a},
            "events": events, "trace": trace}


# ------------------------------------------------------------------------------------------------ the table
R1, R1L, R2, R2L, D1, D1L = "[s0p1]|S", "[s0p1]|L", "[s0p2]|S", "[s0p2]|L", "[01p1]|S", "[01p1]|L"
S2A, S2AL, S2B, S2BL = "[01p1 s0p1]|S", "[01p1 s0p1]|L", "[01p1 s0p2]|S", "[01p1 s0p2]|L"
TB, TBL, TBS = "[s0p1 10p1]|S", "[s0p1 10p1]|L", "[s0p1 s0p1]|S"
S3, S3L = "[s0p1 10p1 s1p1]|S", "[s0p1 10p1 s1p1]|L"
G3, G3P2, G3P2L = "[s0p1][s0p1][s0p1]|SSS", "[s0p1][s0p1][s0p2]|SSS", "[s0p1 10p1 s1p2]|L"
F4, BIG = "[s0p1 s0p1 10p1 s1p1]|L", "big"


def SEP(a, b, ln):
    return "[s0p%d][s0p%d]|%s" % (a, b, ln)


def SEPD(ln):
    return "[01p1][s0p1]|" + ln


def S2SEP(ln):
    return "[01p1 s0p1][s0p1]|" + ln


def SEPD2(ln):
    return "[01p1][s0p2]|" + ln


# player-puck lanes whose other player leans on a wall: once that second island has retired they ride a
# two-contact chunk with a dynamic body A, the retired contact (one or two points) in slot 1
_DYN_RIDERS = [(DYNRIDER, 6), (SEPD("LS"), 6), (SEPD2("LS"), 2), (SEPD("SS"), 4), (SEPD2("SS"), 4)]


class Row:
    """One wave: `lanes` [(class, count)] fill the wave from lane 0 (or `at` {lane: class} places them), idle
    elsewhere; `expect`: the arms / events the row exists for, which the predictor must return for it at `step`.
    same: every lane of a class holds the same scenario.  predict=False: TOI rows (no arm prediction)."""

    def __init__(self, name, lanes=(), expect=(), step=J, at=None, same=False, predict=True, width=64):
        self.name, self.lanes, self.expect, self.step = name, list(lanes), set(expect), step
        self.at, self.same, self.predict, self.width = dict(at or {}), same, predict, width


TABLE = [
    # ---- S3 family
    Row("s3_alone", [(S3L, 3), (S3, 3)], ["s3<1,1>"]),
    Row("s3_riders", [(S3L, 2), (R1, 4), (D1, 3), (R1L, 2), (S3, 1)], ["s3<1,1>", "s3_rider"]),
    Row("s3_s2", [(S3L, 2), (S2A, 3), (S2AL, 2)], ["s3<1,1>", "s3_s2l"]),
    Row("s3_s2_riders", [(S3L, 1), (S3, 1), (S2AL, 2), (S2A, 2), (R1, 3), (D1L, 1)], ["s3<1,1>", "s3_rider", "s3_s2l"]),
    Row("s3short_s2long", [(S3, 3), (S2AL, 3), (R1, 2)], ["s3<1,1>", "s2<1,1>", "shift:s3->two"]),
    Row("s3long_s2short", [(S3L, 3), (S2A, 3)], ["s3<1,1>", "s3_s2l"]),
    Row("s3_p2_rider", [(S3L, 2), (R2, 2), (S2A, 1)], ["s3<0,0>", "s3_rider"]),
    Row("s3_s2p2", [(S3L, 2), (S2B, 2)], ["s3<0,0>", "s3_s2l"]),
    Row("s3_fresh", [(S3L, 2), (S2A, 2), (R1, 2)], ["s3<1,1>"], step=0),
    # ---- general family
    Row("gen_p1", [(G3, 3), (S2A, 2), (R1, 2)], ["vgen<reg,1>"]),
    Row("gen_s3_beside_tb", [(S3L, 2), (TB, 2), (S3, 1)], ["vgen<reg,1>"]),
    Row("gen_p0", [(G3P2, 3), (R1, 2)], ["vgen<reg,0>"]),
    Row("gen_p0_island", [(G3P2L, 2), (S2A, 2)], ["vgen<reg,0>"]),
    Row("gen_four", [(F4, 2), (S2A, 3), (R1, 3), (S2AL, 1)], ["vgen<reg,1>"]),
    Row("gen_hbm", [(BIG, 2), (S2AL, 2), (R1, 2), (S3L, 1)], ["hbm"], step=None),
    Row("gen_to_two", [(S2SEP("SL"), 3), (S2AL, 3), (G3, 2)],
        ["vgen<reg,1>", "s2<1,1>", "shift:gen->two", "swap", "rider_retired_slot1", "retire"]),
    # a rider with a DYNAMIC body A whose slot 1 holds a retired contact (its dummy contact-1 solve reads a moving
    # body, so an unrestored slot 1 changes the next step's warm start), in the S2 and in the aliased chunk.  The
    # short S3 lanes sit beside lanes of another two-contact shape, so the wave starts in the general family and
    # stays there until they are done: by then the riders' second island has retired
    Row("rider_dyn_retired_slot1_s2", _DYN_RIDERS + [(S3, 4), (S2AL, 3)],
        ["vgen<reg,0>", "s2<1,1>", "shift:gen->two", "rider_dyn_retired_slot1"]),
    Row("rider_dyn_retired_slot1_alias", _DYN_RIDERS + [(S3, 4), (TBL, 2), (S2AL, 1)],
        ["vgen<reg,0>", "alias<1,1>", "shift:gen->two", "rider_dyn_retired_slot1"]),
    Row("gen_to_two_s2sep", [(S2SEP("LS"), 4), (S2SEP("SS"), 2)], ["vgen<reg,1>", "s2<1,1>", "shift:gen->two"]),
    # ---- S2 chunk
    Row("s2_11", [(S2A, 3), (S2AL, 3)], ["s2<1,1>"]),
    Row("s2_11_riders", [(S2A, 2), (S2AL, 3), (R1, 3), (D1, 2), (R1L, 2), (D1L, 1)], ["s2<1,1>"]),
    Row("s2_01_p2_riders", [(S2AL, 3), (S2A, 1), (R2, 3), (R2L, 2)], ["s2<0,1>"]),
    Row("s2_12", [(S2B, 3), (S2BL, 3)], ["s2<1,2>"]),
    Row("s2_12_riders", [(S2B, 2), (S2BL, 3), (R1, 3), (D1L, 1)], ["s2<1,2>"]),
    Row("s2_02_p2_riders", [(S2BL, 3), (R2, 2), (R2L, 2)], ["s2<0,2>"]),
    Row("s2_fresh", [(S2A, 3), (S2AL, 2), (R1, 2)], ["s2<1,1>"], step=0),
    # ---- aliased chunk
    Row("alias_11_s2_tb", [(S2AL, 2), (TBL, 2), (S2A, 1), (TB, 1)], ["alias<1,1>"]),
    Row("alias_10_s2_points", [(S2AL, 2), (S2BL, 2), (S2A, 1), (S2B, 1)], ["alias<1,0>"]),
    Row("alias_01", [(S2AL, 2), (TBL, 2), (R2, 2), (R2L, 1)], ["alias<0,1>"]),
    Row("alias_00", [(S2BL, 2), (S2AL, 2), (R2L, 2), (TBL, 1)], ["alias<0,0>"]),
    Row("alias_tb_only", [(TBL, 3), (TB, 2), (TBS, 2)], ["alias<1,1>"]),
    Row("alias_tb_riders", [(TBL, 2), (R1, 3), (D1L, 2)], ["alias<1,1>"]),
    # ---- generic two-contact chunk
    Row("vtwo_11_sep_riders", [(SEP(1, 1, "LL"), 2), (SEP(1, 1, "SS"), 3), (R1, 3), (D1, 1)], ["vtwo<1,1,false>"]),
    Row("vtwo_11_sepd", [(SEPD("SS"), 3), (SEPD("LS"), 2), (SEP(1, 1, "SS"), 2)], ["vtwo<1,1,false>"]),
    Row("vtwo_12", [(SEP(1, 2, "SS"), 3), (SEP(1, 2, "LS"), 3), (R1, 2)], ["vtwo<1,2,false>"]),
    Row("vtwo_21", [(SEP(2, 1, "SS"), 3), (SEP(2, 1, "SL"), 3), (R2, 2)], ["vtwo<2,1,false>"]),
    Row("vtwo_22", [(SEP(2, 2, "SS"), 4), (R2, 2)], ["vtwo<2,2,false>"]),
    Row("vtwo_00", [(SEP(1, 1, "SS"), 2), (SEP(2, 2, "SS"), 2), (SEP(1, 2, "SS"), 1), (S2A, 1)], ["vtwo<0,0,false>"]),
    Row("vtwo_kg", [(SEP(1, 1, "SL"), 3), (SEP(1, 1, "LL"), 2)], ["vtwo<1,1,false>", "vtwo<0,0,true>", "retire"]),
    Row("vtwo_kg_beside_s2", [(SEP(1, 1, "SL"), 2), (S2AL, 2), (SEPD("SL"), 2)], ["vtwo<0,0,true>", "retire"]),
    # ---- one-contact family
    Row("vone_sa_p1", [(R1, 4), (R1L, 3)], ["vone<true,1>"]),
    Row("vone_sa_p2", [(R2, 3), (R2L, 3)], ["vone<true,2>"]),
    Row("vone_sa_p0", [(R1L, 2), (R2L, 2), (R1, 2)], ["vone<true,0>"]),
    Row("vone_dyn_p1", [(D1, 3), (D1L, 3), (R1L, 2)], ["vone<false,1>"]),
    Row("vone_dyn_p0", [(D1L, 3), (R2L, 2), (R1, 1)], ["vone<false,0>"]),
    Row("vone_fresh", [(D1, 3), (D1L, 2), (R1, 2), (R2, 1)], ["vone<false,0>"], step=0),
    # ---- late events
    Row("two_to_one_swap", [(SEP(1, 1, "SL"), 3), (SEP(1, 1, "SS"), 2), (R1, 2)],
        ["vtwo<1,1,false>", "vone<true,1>", "shift:two->one", "swap", "retire"]),
    Row("two_to_one_first_survives", [(SEP(1, 1, "LS"), 3), (SEP(1, 2, "LS"), 2)], ["shift:two->one", "retire"]),
    Row("two_to_one_dyn", [(SEPD("SL"), 2), (SEPD("LS"), 2), (S2A, 2)], ["shift:two->one", "retire"]),
    Row("s2sep_down", [(S2SEP("SL"), 2), (S2SEP("LS"), 2), (S2SEP("SS"), 2)], ["vgen<reg,1>", "retire"]),
    # ---- lane placement
    Row("full_wave_one_s2_long", [(S2AL, 64)], ["s2<1,1>"], same=True),
    Row("one_live_lane", [], ["s2<1,1>"], at={17: S2AL}),
]
# every multi-contact class once at lane 0, once mid-wave, once at lane 63
_PLACED = [S2A, S2AL, S2B, S2BL, TB, TBL, TBS, SEP(1, 1, "SS"), SEP(1, 1, "LL"), SEP(1, 2, "SS"), SEP(2, 1, "SS"),
           SEP(2, 2, "SS"), SEPD("SS"), S2SEP("SS"), S3, S3L, G3, G3P2, F4, BIG]
for _i, _c in enumerate(_PLACED):
    TABLE.append(Row("placed_%02d" % _i, at={0: _c, 31: _PLACED[(_i + 1) % len(_PLACED)],
                                             63: _PLACED[(_i + 2) % len(_PLACED)], 5: R1, 40: D1}))
TABLE += [
    # ---- TOI (no arm prediction: the event counts are asserted)
    Row("toi_every_lane", [("toi1", 64)], predict=False),
    Row("toi_single_lane", at={29: "toi1"}, predict=False),
    Row("toi_2_and_3_events", at={0: "toi2", 7: "toi3", 33: "toi2", 63: "toi3", 20: "toim2"}, predict=False),
    # ---- the final partial wave
    Row("tail_37", [(S3L, 2), (S2AL, 3), (S2A, 3), (R1, 20), (D1, 8), (S3, 1)], ["s3<1,1>", "s3_rider", "s3_s2l"],
        width=37),
]


class Batch:
    """The composed batch: which scenario sits in which arena, wave by wave in TABLE order."""

    def __init__(self, zoo):
        self.zoo = zoo
        self.idx, self.rows, self.step = [], [], []
        for ri, row in enumerate(TABLE):
            step = row.step
            if step is None:  # BIG lanes: whatever step the harvest found them at
                step = min(t for (t, c) in zoo.pool if c == BIG)
            cls = ["idle"] * row.width
            lane = 0
            for c, k in row.lanes:
                cls[lane:lane + k] = [c] * k
                lane += k
            for l, c in row.at.items():
                cls[l] = c
            assert lane <= row.width and len(cls) == row.width, row.name
            seen = {}
            for c in cls:
                pool = zoo.pool.get((step, c))
                assert pool, "no scenario of class %r at step %d (row %s)" % (c, step, row.name)
                k = seen.get(c, 0)
                seen[c] = k + (0 if row.same else 1)
                self.idx.append(pool[(k + ri) % len(pool)] if c != "idle" else pool[k % len(pool)])
            self.rows += [ri] * row.width
            self.step.append(step)
        self.idx = np.array(self.idx)
        self.n = len(self.idx)
        d = zoo.d
        self.state, self.aux = d["state"][self.idx], d["aux"][self.idx]
        self.actions = np.ascontiguousarray(d["actions"][self.idx].transpose(1, 0, 2))  # [K, n, 8]
        self.toi = d["toi"][self.idx].astype(np.int64)  # [n, K]
        # solves the kernel routes to the HBM slot file: lanes with more island contacts than register slots, and
        # TOI mini-islands with more contacts than the TOI register slots
        self.large = int((d["ncont"][self.idx] > 4).sum() + d["toi_big"][self.idx].sum())

    def wave_lanes(self, ri, t):
        a = np.nonzero(np.array(self.rows) == ri)[0]
        return [self.zoo.lane(self.idx[i], t) for i in a]

    def predict_row(self, ri, strict=True):
        return predict(self.wave_lanes(ri, self.step[ri]), strict=strict)

    def describe(self, arena, t):
        """Failure context of one arena at step t: its wave's table row, the lane's scenario, and the arms predicted
        for the wave at that step and the one before."""
        ri = self.rows[arena]
        out = "wave %d row %r (label step %s) lane %d scenario %d class %s" % (
            ri, TABLE[ri].name, self.step[ri], arena - self.rows.index(ri), self.idx[arena],
            self.zoo.cls[self.idx[arena]][t])
        for u in range(max(t - 1, 0), t + 1):  # a wrong impulse shows a step later, in the warm start
            p = predict(self.wave_lanes(ri, u), strict=False)
            out += "\n  wave arms at step %d: %s events %s" % (u, p["trace"], sorted(p["events"]))
        return out


# ------------------------------------------------------------------------------------------------ the harvest
HARVEST = dict(seed=20260, n=8192, preroll=300, windows=400)


def _sweep(n, preroll, windows, seed, want):
    """Run the strong-vs-strong source, replay every K-step window under the probe and hand each replayed
    candidate's per-step classes to want(classes, labels_row) -> bool (keep)."""
    import oracle as O

    O.build()
    src = O.OracleVec(n, policies=("strong", "strong"), auto_reset=True, seed=seed)
    for _ in range(preroll):
        src.step()
    kept = {f: [] for f in ("state", "aux", "actions") + LABEL_FIELDS}
    for _ in range(windows):
        st, aux = src.get_state()
        acts = np.stack([src.step()["actions"] for _ in range(K)])
        rec, ok = probe_replay(st, aux, acts)
        lab = labels_of(rec)
        for i in np.nonzero(ok)[0]:
            row = {f: lab[f][i] for f in LABEL_FIELDS}
            cls = [class_of(row["shape"][t], row["cur"][t], row["toi"][t]) for t in range(K)]
            if want(cls, row):
                kept["state"].append(st[i])
                kept["aux"].append(aux[i])
                kept["actions"].append(acts[:, i])
                for f in LABEL_FIELDS:
                    kept[f].append(row[f])
    src.close()
    return {f: np.stack(v) for f, v in kept.items()}


def save_fixture(d, path=FIXTURE):
    """np.load-able archive with fixed member order and timestamps: the same data give the same bytes."""
    with zipfile.ZipFile(path, "w") as z:
        for name in sorted(d):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(d[name]), allow_pickle=False)
            zi = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            z.writestr(zi, buf.getvalue(), compresslevel=9)


def harvest(path=FIXTURE, **kw):
    """The committed fixture from its seed: every replayed class (no M island) at the label step J up to QUOTA_J
    scenarios, at step 0 (fresh contacts, no warm start) up to QUOTA_0, and TOI steps by event count."""
    cfg = dict(HARVEST, **kw)
    count = {}

    def want(cls, row):
        keys = [((t, cls[t]), q) for t, q in ((J, QUOTA_J), (0, QUOTA_0)) if "M" not in cls[t].split("|")[-1]]
        if row["toi"][J]:
            keys.append(((J, "toi%d" % min(int(row["toi"][J]), 3)), QUOTA_TOI))
        if row["toi_n2"][J]:
            keys.append(((J, "toim2"), QUOTA_TOI))
        if row["toi_big"][J]:
            keys.append(((J, "toibig"), QUOTA_TOI))
        if is_dynrider(cls, row["shape"]):
            keys.append(((J, DYNRIDER), QUOTA_J))
        for t in range(K):  # lanes with more island contacts than register slots are rare: taken at any step
            if row["ncont"][t] > 4 and "M" not in cls[t].split("|")[-1]:
                keys.append(((t, "big"), QUOTA_TOI))
        if not any(count.get(k, 0) < q for k, q in keys):
            return False
        for k, _ in keys:
            count[k] = count.get(k, 0) + 1
        return True

    d = _sweep(cfg["n"], cfg["preroll"], cfg["windows"], cfg["seed"], want)
    d = _splice_big(d, count)
    save_fixture(d, path)
    return d, count


def _splice_big(d, count):
    """Lanes with more island contacts than the kernel's 4 register slots.  The strong-vs-strong run did not show
    one in 13 million replayed lane-steps, so the harvest composes them from its own scenarios: a scenario with a
    four-contact island (puck in a corner, one player on it) takes the OTHER player's state rows and actions from
    a second scenario, and is kept if its replay shows that player in a contact of its own at step J (the two
    players' islands share no body, so neither disturbs the other)."""
    have = sum(v for (t, c), v in count.items() if c == BIG)
    if have >= QUOTA_TOI:
        return d
    n = d["state"].shape[0]
    four = [i for i in range(n) if d["shape"][i, J].count(b" ") >= 3 and d["ncont"][i, J] == 4]
    cand = {f: [] for f in ("state", "aux", "actions")}
    for x in four:
        for y in range(n):
            for pl in (0, 1):
                st, ac = d["state"][x].copy(), d["actions"][x].copy()
                st[6 * pl:6 * pl + 6] = d["state"][y, 6 * pl:6 * pl + 6]
                ac[:, 4 * pl:4 * pl + 4] = d["actions"][y, :, 4 * pl:4 * pl + 4]
                cand["state"].append(st)
                cand["aux"].append(d["aux"][x])
                cand["actions"].append(ac)
    cand = {f: np.stack(v) for f, v in cand.items()}
    rec, ok = probe_replay(cand["state"], cand["aux"], np.ascontiguousarray(cand["actions"].transpose(1, 0, 2)))
    lab = labels_of(rec)
    keep = []
    for i in np.nonzero(ok)[0]:
        if have + len(keep) >= QUOTA_TOI:
            break
        if lab["ncont"][i, J] > 4 and "M" not in letters(lab["cur"][i, J]):
            keep.append(i)
            count[(J, BIG)] = count.get((J, BIG), 0) + 1
    out = {f: np.concatenate([d[f], cand[f][keep]]) for f in cand}
    out.update({f: np.concatenate([d[f], lab[f][keep]]) for f in LABEL_FIELDS})
    return out


QUOTA_J, QUOTA_0, QUOTA_TOI = 6, 2, 4

if __name__ == "__main__":
    if "--harvest" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else FIXTURE
        d, count = harvest(out)
        for k in sorted(count):
            print("%d %-44s %d" % (k[0], k[1], count[k]))
        print("%d scenarios, %d bytes -> %s" % (d["state"].shape[0], os.path.getsize(out), out))
