"""A batch whose waves are certain to overflow the cooperative work list of both drains (hk_collide.h
collide_near_wave, hk_world.h toi_drain_wave).

A wave lists up to WAVE_Q (lane, pair) items per round; a wave with more goes round again, and a partial wave deals
the list to fewer than 64 workers.  The batch is 101 arenas: a full wave whose every lane lists at least 3 items in
each drain at step 0 (192 > 128), and a wave of 37 lanes with at least 4 each (148 > 128, fewer than 64 workers).

Certainty does not restate the kernel.  Both far tests reject a static-dynamic pair only when a box that contains
body B's centre of mass is farther than `reach` from the static fixture's AABB (a player's core box contains its
COM; the TOI sweep box contains the sweep's start, the state's COM, which the pre-solve laws do not move with no
puck held).  So the pair is listed whenever the state's COM lies within reach - SLACK of fx_aabb[fA], reach being
the Collide test's (circle B: total radius + margin, polygon B: twice the total radius + margin) or the TOI test's
(max(slop, total - 3 slop) + slop / 4 + margin).  A dynamic-dynamic pair is listed in Collide whenever the COM
distance is below the sum of the two rcore.  near_counts() evaluates exactly that, in float64, from the compiled
scene data.

The states: the puck in a rink corner within its radius of a wall and a post (two items in both lists), a player
with its COM inside its own goal fixture's AABB (one each), and in some lanes a player's COM on the puck (Collide
items).  Offsets are seeded per lane and keep the condition.  numpy only.
"""
import ast
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE_INC = os.path.join(ROOT, "hockey-env_amd", "csrc", "hk_scene_data.inc")

N_FULL, N_PART = 64, 37
N = N_FULL + N_PART
K = 3
WAVE_Q = 128          # hk_body.h kToiQ
MIN_FULL, MIN_PART = 3, 4
SLACK = 0.01          # the condition's distance from the far tests' thresholds
# Box2D / kernel constants the far tests' reaches are made of (hk_core.h)
SLOP, FAR_MARGIN, TOI_MARGIN = 0.005, 0.005, 0.005
B_P1, B_P2, B_PK = 0, 1, 2
F_WT, F_WB, F_PLT, F_PLB, F_PRT, F_PRB, F_G1, F_G2 = 0, 1, 2, 3, 4, 5, 7, 9
HOME = ((2.0, 4.0), (8.0, 4.0))


def scene():
    """hk_scene_data.inc as nested lists, keyed by the fields of hk_core.h Scene this module uses."""
    with open(SCENE_INC) as f:
        text = "".join(line for line in f if not line.startswith("//"))
    text = re.sub(r"-?0x[0-9a-f.]+p[+-]\d+f", lambda m: repr(float.fromhex(m.group(0)[:-1])), text)
    s = ast.literal_eval(text.replace("{", "[").replace("}", "]"))
    fx = s[0]
    return {"radius": np.array([f[8] for f in fx]), "circle": np.array([f[0] for f in fx]),
            "lc": np.array([s[5], s[6]]).T, "pairA": np.array(s[9]), "pairB": np.array(s[10]),
            "pbodyA": np.array(s[11]), "pbodyB": np.array(s[12]), "sensor": np.array(s[13]),
            "fx_aabb": np.array(s[18]), "rcore": np.array(s[19])}


def com(state, S):
    """[N, 3, 2] float64 centres of mass of the raw state's bodies: origin + R(angle) * local centre."""
    b = np.asarray(state, np.float64).reshape(-1, 3, 6)
    c, s = np.cos(b[:, :, 2]), np.sin(b[:, :, 2])
    lx, ly = S["lc"][:, 0], S["lc"][:, 1]
    return np.stack([b[:, :, 0] + c * lx - s * ly, b[:, :, 1] + s * lx + c * ly], axis=2)


def near_counts(state, S):
    """Per arena, how many pairs are certain to be listed at step 0: (Collide list, TOI list)."""
    c = com(state, S)
    collide = np.zeros(len(c), np.int64)
    toi = np.zeros(len(c), np.int64)
    for p in range(len(S["pairA"])):
        fA, fB, bA, bB = S["pairA"][p], S["pairB"][p], S["pbodyA"][p], S["pbodyB"][p]
        total = S["radius"][fA] + S["radius"][fB]
        if bA >= 3:
            box = S["fx_aabb"][fA]
            x, y = c[:, bB, 0], c[:, bB, 1]
            gap = np.maximum(np.maximum(box[0] - x, x - box[2]), np.maximum(box[1] - y, y - box[3]))
            reach = total + TOI_MARGIN if S["circle"][fB] else 2.0 * total + FAR_MARGIN
            collide += gap <= reach - SLACK
            if not S["sensor"][p]:
                reach = max(SLOP, total - 3.0 * SLOP) + 0.25 * SLOP + TOI_MARGIN
                toi += gap <= reach - SLACK
        else:
            d = np.hypot(c[:, bA, 0] - c[:, bB, 0], c[:, bA, 1] - c[:, bB, 1])
            collide += d < S["rcore"][bA] + S["rcore"][bB] - SLACK
    return collide, toi


def _origin(cx, cy, angle, lc):
    c, s = np.cos(angle), np.sin(angle)
    return cx - (c * lc[0] - s * lc[1]), cy - (s * lc[0] + c * lc[1])


class Batch:
    """state[N,18], aux[N,5], actions[K,N,8] and the per-lane kind: 'all' (puck corner, both players in goal),
    'p1' / 'p2' (only that player in its goal, the other parked or, every other such lane, on the puck)."""

    def __init__(self, seed=0):
        S = scene()
        rng = np.random.default_rng(seed)
        box = S["fx_aabb"]
        u = rng.uniform
        rows, kinds = [], []
        for i in range(N):
            kind = "all" if i >= N_FULL else ("all", "p1", "p2")[i % 3]
            left, top = bool(rng.integers(2)), bool(rng.integers(2))
            post = box[(F_PLT if top else F_PLB) if left else (F_PRT if top else F_PRB)]
            d1, d2 = u(0.17, 0.2), u(0.17, 0.2)  # inside the TOI reach of the puck's pairs less SLACK (0.2079)
            pkx = post[2] + d1 if left else post[0] - d1
            pky = box[F_WT][1] - d2 if top else box[F_WB][3] + d2
            pk = [pkx, pky, 0.0, u(-3, 3), u(-3, 3), u(-20, 20)]
            body = []
            for b, goal in ((B_P1, F_G1), (B_P2, F_G2)):
                a = u(-0.4, 0.4)
                if kind in ("all", ("p1", "p2")[b]):
                    g = box[goal]  # COM inside the goal fixture's AABB, 3 cm from its sides
                    cx, cy = u(g[0] + 0.03, g[2] - 0.03), u(g[1] + 0.6, g[3] - 0.6)
                elif (i // 3) % 2:  # COM on the puck: within 0.3 m < rcore of the puck's centre
                    r, th = u(0.0, 0.3), u(0, 2 * np.pi)
                    cx, cy = pkx + r * np.cos(th), pky + r * np.sin(th)
                else:
                    cx, cy = HOME[b][0] + u(-0.3, 0.3), HOME[b][1] + u(-1, 1)
                x, y = _origin(cx, cy, a, S["lc"][b])
                body.append([x, y, a, u(-2, 2), u(-2, 2), u(-3, 3)])
            rows.append(np.concatenate([body[0], body[1], pk]))
            kinds.append(kind)
        self.n = N
        self.kind = np.array(kinds)
        self.state = np.array(rows, np.float32)
        self.aux = np.zeros((N, 5), np.int32)
        self.actions = rng.uniform(-1, 1, (K, N, 8)).astype(np.float32)
        for a in (self.state, self.aux, self.actions):
            a.setflags(write=False)

    def describe(self, i, t):
        return "arena %d (wave %d lane %d, kind %s), step %d, state %s" % (
            i, i // 64, i % 64, self.kind[i], t, self.state[i].tolist())
