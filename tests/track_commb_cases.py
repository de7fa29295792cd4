"""The lists a track table's Comm-B side is checked on (tests/test_track_commb_host.py on the CPU mirror,
tests/test_gpu_track_commb.py on the device).  A case is dict(name, frames, recs, commb, claim): a FRAME_DTYPE list, its
adsb_modes_rec and stateless adsb_commb_rec records (the models', so no library call is needed to build a case), and the
claim the list is there to show.  claims_hold() asserts every claim against the MODEL's result, so a list cannot quietly
stop showing it.

Aircraft with ADS-B are given as DF17 frames of kind SELF, their Comm-B replies as DF20 frames of kind KNOWN with the
same address, as adsb_modes_of would resolve them from the parity."""
import math

import numpy as np

from tests import commb_model as CM
from tests import modes_model as MM
from tests import track_commb_model as T

SPS = 0.5e-6
STEP = 2000                                  # samples between frames: 1 ms


def vel_frame(icao, st=1, **raw):
    """A DF17 TC 19 frame of subtype st; raw: ME fields by (first bit, width) names of the header"""
    fields = {"dew": (13, 1), "vew": (14, 10), "dns": (24, 1), "vns": (25, 10), "status": (13, 1), "heading": (14, 10),
              "as_type": (24, 1), "airspeed": (25, 10), "vrsrc": (35, 1), "svr": (36, 1), "vr": (37, 9)}
    me = 19 << 51 | st << 48
    for name, value in raw.items():
        first, width = fields[name]
        assert 0 <= value < 1 << width, (name, value)
        me |= value << (56 - first - width)
    return bytes([0x8D, icao >> 16 & 0xFF, icao >> 8 & 0xFF, icao & 0xFF]) + me.to_bytes(7, "big") + b"\0\0\0"


def ground_frame(icao, ew, ns, vr=None, st=1):
    """ST 1 (or 2) with the signed components in kt (multiples of 4 for ST 2) and the vertical rate in ft/min (a
    multiple of 64; None: not given)"""
    k = 4 if st == 2 else 1
    raw = dict(dew=int(ew < 0), vew=abs(ew) // k + 1, dns=int(ns < 0), vns=abs(ns) // k + 1)
    if vr is not None:
        raw.update(svr=int(vr < 0), vr=abs(vr) // 64 + 1, vrsrc=1)
    return vel_frame(icao, st, **raw)


def air_frame(icao, heading=None, airspeed=None, tas=1, vr=None, st=3):
    """ST 3 (or 4): the 10-bit heading, the airspeed in kt (a multiple of 4 for ST 4) and its type"""
    k = 4 if st == 4 else 1
    raw = {}
    if heading is not None:
        raw.update(status=1, heading=heading)
    if airspeed is not None:
        raw.update(airspeed=airspeed // k + 1, as_type=tas)
    if vr is not None:
        raw.update(svr=int(vr < 0), vr=abs(vr) // 64 + 1, vrsrc=1)
    return vel_frame(icao, st, **raw)


def other_frame(icao, tc=4):
    """A DF17 frame that is no velocity message"""
    return bytes([0x8D, icao >> 16 & 0xFF, icao >> 8 & 0xFF, icao & 0xFF, tc << 3]) + b"\x20" * 6 + b"\0\0\0"


def reply(mb, df=20):
    return CM.frame(mb, df=df)


def build(name, items, claim=None, offsets=None):
    """items: [(14 bytes, address, kind)] in list order -> the case"""
    n = len(items)
    frames = np.zeros(n, dtype=CM.FRAME_DTYPE)
    recs = np.zeros(n, dtype=MM.REC_DTYPE)
    for j, (msg, address, kind) in enumerate(items):
        frames["bytes"][j] = np.frombuffer(bytes(msg), dtype=np.uint8)
        recs["address"][j], recs["df"][j], recs["kind"][j] = address, msg[0] >> 3, kind
    frames["offset"] = np.arange(n) * STEP if offsets is None else np.asarray(offsets)
    frames["fixed_bit"] = 0xFF
    return dict(name=name, frames=frames, recs=recs, commb=CM.commb(frames)["recs"], claim=claim)


def run_model(case, cuts=(), **table):
    """The model over the case, cut at the given list positions -> (frame_commb, records, the Table)"""
    t = T.Table(**table)
    edges = [0] + list(cuts) + [len(case["frames"])]
    outs = [t.update(case["frames"][a:b], case["recs"][a:b], case["commb"][a:b]) for a, b in zip(edges, edges[1:])]
    return np.concatenate(outs) if outs else np.zeros(0, dtype=CM.REC_DTYPE), t.records(), t


# ---- the seeded realistic mix ------------------------------------------------------------------------------------------
def realistic(rng):
    """One aircraft state: ground vector (150-540 kt, any track), wind up to 70 kt, vertical rate 0 in three quarters
    of the draws and within +-3000 ft/min otherwise -> dict"""
    gs, track = rng.uniform(150, 540), rng.uniform(0, 360)
    wind, wdir = rng.uniform(0, 70), rng.uniform(0, 360)
    ew, ns = gs * math.sin(math.radians(track)), gs * math.cos(math.radians(track))
    aew, ans = ew - wind * math.sin(math.radians(wdir)), ns - wind * math.cos(math.radians(wdir))
    vr = 0 if rng.random() < 0.75 else int(rng.integers(-3000, 3001))
    return dict(ew=int(round(ew)), ns=int(round(ns)), gs=gs, track=track, tas=math.hypot(aew, ans),
                heading=math.degrees(math.atan2(aew, ans)) % 360, vr=vr)


def payload_50(rng, s):
    """All five status bits: roll within 10 degrees, the true track, ground speed, a small track rate, true airspeed"""
    track = int(round(s["track"] / (90 / 512))) % 2048
    return CM.mb_50(roll=int(rng.integers(-57, 58)), track=track - 2048 if track >= 1024 else track,
                    gs=int(round(s["gs"] / 2)), rate=int(rng.integers(-8, 9)), tas=int(round(s["tas"] / 2)))


def payload_60(rng, s):
    """All five status bits: magnetic heading (variation within 10 degrees), IAS and Mach from the true airspeed at a
    random level, both vertical rates within 100 ft/min of the true one"""
    heading = int(round(((s["heading"] + rng.uniform(-10, 10)) % 360) / (90 / 512))) % 2048
    ias = int(round(s["tas"] * rng.uniform(0.6, 1.0)))
    mach = int(round(s["tas"] / rng.uniform(573, 661) / 0.004))
    rate = lambda: int(round((s["vr"] + rng.uniform(-100, 100)) / 32))
    return CM.mb_60(heading=heading - 2048 if heading >= 1024 else heading, ias=ias, mach=mach, baro=rate(), inertial=rate())


def mix(n_each=4000, seed=20, n_aircraft=64):
    """n_each payloads of each register, every one directly behind an ST 1 velocity message of its aircraft that says
    the same state.  A draw whose payload is no candidate of its own register (a true airspeed above 500 kt, say) is
    drawn again.  -> the case; case["truth"][j] is the true register of reply j (0 for the velocity frames)"""
    rng = np.random.default_rng(seed)
    items, truth = [], []
    for k in range(2 * n_each):
        bds = 0x50 if k % 2 == 0 else 0x60
        icao = 0x400000 + int(rng.integers(0, n_aircraft))
        while True:
            s = realistic(rng)
            mb = (payload_50 if bds == 0x50 else payload_60)(rng, s)
            if CM.TESTS[bds](CM.MB(mb)):
                break
        items += [(ground_frame(icao, s["ew"], s["ns"], vr=s["vr"] // 64 * 64 if s["vr"] >= 0 else -(-s["vr"] // 64 * 64)),
                   icao, T.SELF), (reply(mb, df=20 + k % 4 // 2), icao, T.KNOWN)]
        truth += [0, bds]
    case = build(f"the realistic mix, {n_each} payloads of each register", items, claim=("mix", n_each))
    case["truth"] = np.array(truth)
    return case


def mix_tally(case, out):
    """-> dict of counts per true register: payloads, ambiguous as {5,0; 6,0}, settled right, left ambiguous, wrong"""
    tally = {}
    for bds in (0x50, 0x60):
        mine = case["truth"] == bds
        amb = mine & (case["commb"]["state"] == T.AMBIGUOUS) & (case["commb"]["candidates"] == T.C50 | T.C60)
        settled = amb & (out["state"] == T.SETTLED)
        tally[bds] = dict(payloads=int(mine.sum()), ambiguous=int(amb.sum()), right=int((settled & (out["bds"] == bds)).sum()),
                          left=int((amb & (out["state"] == T.AMBIGUOUS)).sum()),
                          wrong=int((settled & (out["bds"] != bds)).sum()))
    return tally


# ---- constructed lists -------------------------------------------------------------------------------------------------
A, B, C = 0x4B1234, 0x3C6655, 0x0000A1
# reads as 5,0 and as 6,0.  As 5,0: track 253.8 degrees, 430 kt, TAS 360 kt.  As 6,0 its two vertical rates are -640
# and +5760 ft/min: a reference that says 430 kt at 254 degrees in level flight settles it to 5,0
BOTH = CM.mb_50(roll=-33, track=-1024 + 420, gs=215, rate=-20, tas=180)
AGREES = dict(ew=-413, ns=-120, vr=0)                 # with BOTH read as 5,0
OPPOSES = dict(ew=200, ns=200, vr=5760)               # 283 kt to the north-east, climbing as BOTH read as 6,0 says


def registers():
    """every state and every register on one aircraft, then again on a second one in another order"""
    from tests import commb_cases as K
    msgs = [bytes(m) for m in K.KNOWN_FRAMES] + [reply(b"\0" * 7), reply(b"\xff" * 7), reply(BOTH),
                                                 reply(CM.mb_of({}, ones=[1, 7, 14, 20])), reply(K.FULL[0x40]),
                                                 reply(K.FULL[0x60]), reply(CM.mb_30(ara=0x2A81, rac=3, tti=1, tid=99)),
                                                 reply(CM.mb_17([7, 9, 16, 24]))]
    items = [(m, A, T.KNOWN) for m in msgs] + [(m, B, T.KNOWN) for m in reversed(msgs)]
    items += [(other_frame(C), C, T.SELF), (K.KNOWN_FRAMES[1], C, T.UNKNOWN), (reply(BOTH), 0, T.PARITY)]
    return build("every state and register, two orders; rejected frames", items, claim=("registers",))


def twelve():
    """reference -> ambiguous -> reference -> ambiguous on one aircraft, other aircraft in between"""
    items = [(other_frame(B), B, T.SELF), (ground_frame(A, **AGREES), A, T.SELF), (reply(BOTH), B, T.KNOWN),
             (reply(BOTH), A, T.KNOWN), (other_frame(A), A, T.SELF), (ground_frame(B, **OPPOSES), B, T.SELF),
             (ground_frame(A, **OPPOSES), A, T.SELF), (reply(BOTH), B, T.KNOWN), (reply(BOTH), A, T.KNOWN),
             (ground_frame(A, **AGREES), A, T.SELF), (reply(CM.mb_17([7, 24])), A, T.KNOWN), (reply(BOTH), A, T.KNOWN)]
    want = {2: (T.AMBIGUOUS, 0), 3: (T.SETTLED, 0x50), 7: (T.AMBIGUOUS, 0), 8: (T.AMBIGUOUS, 0), 11: (T.SETTLED, 0x50)}
    return build("reference, ambiguous, another reference, ambiguous", items, claim=("frames", want))


def between():
    """two velocity frames with the ambiguous frame between them: the later one must not be used"""
    items = [(ground_frame(A, **OPPOSES), A, T.SELF), (reply(BOTH), A, T.KNOWN), (ground_frame(A, **AGREES), A, T.SELF)]
    return build("the later velocity frame is not used", items, claim=("frames", {1: (T.AMBIGUOUS, 0)}))


def list_wins():
    """for use after held(): the list's own reference wins over the held one"""
    items = [(ground_frame(A, **OPPOSES), A, T.SELF), (reply(BOTH), A, T.KNOWN)]
    return build("the list's reference wins", items, offsets=[40 * STEP, 41 * STEP])


def held():
    """an update that only leaves a velocity behind, and one that only has the reply"""
    first = build("a velocity message alone", [(ground_frame(A, **AGREES), A, T.SELF)])
    second = build("the reply alone", [(reply(BOTH), A, T.KNOWN)], offsets=[20 * STEP])
    return first, second


def boundary(variant):
    """One aircraft whose segment crosses sorted position 256 (a lower address fills 0..199): the reference is the last
    frame before the boundary (0), the first after it (1), or directly before the ambiguous frame at an equal offset
    with the pair across the boundary (2)"""
    items = [(other_frame(C), C, T.SELF) for _ in range(200)]
    ref = {0: 255, 1: 256, 2: 255}[variant] - 200
    amb = {0: 300, 1: 257, 2: 256}[variant] - 200
    mine = [(other_frame(A), A, T.SELF) for _ in range(120)]
    mine[ref] = (ground_frame(A, **AGREES), A, T.SELF)
    mine[amb] = (reply(BOTH), A, T.KNOWN)
    mine[5] = (ground_frame(A, **OPPOSES), A, T.SELF)                         # an older one, superseded
    offsets = np.arange(320) * STEP
    if variant == 2:
        offsets[200 + amb] = offsets[200 + ref]
    case = build(f"a segment across the 256-thread boundary, variant {variant}", items + mine, offsets=offsets,
                 claim=("frames", {200 + amb: (T.SETTLED, 0x50)}))
    return case


def no_commb():
    items = [(ground_frame(A, **AGREES), A, T.SELF), (other_frame(B), B, T.SELF), (MM.all_call(C).ljust(14, b"\0"), C, T.SELF)]
    return build("no Comm-B frame", items, claim=("counts", 0, 0))


def none_ambiguous():
    from tests import commb_cases as K
    items = [(ground_frame(A, **AGREES), A, T.SELF)] + [(bytes(m), A, T.KNOWN) for m in K.KNOWN_FRAMES]
    return build("no ambiguous frame", items, claim=("counts", len(K.KNOWN_FRAMES), 0))


def other_candidate_sets():
    """every ambiguous candidate set other than {5,0; 6,0} behind a reference that agrees with its 5,0 reading"""
    from tests import commb_cases as K
    _, fr, claim = K.ambiguous()
    items = [(ground_frame(A, **AGREES), A, T.SELF)]
    items += [(fr["bytes"][j].tobytes(), A, T.KNOWN) for j, (_, c) in enumerate(claim[1]) if c != T.C50 | T.C60]
    return build("other candidate sets stay ambiguous", items, claim=("stay",))


def sized(n, seed=5):
    """n frames of the mix's kind over a few aircraft, with rejected and non-Comm-B frames mixed in"""
    rng = np.random.default_rng(seed + n)
    base = mix(n_each=max(n // 3, 2), seed=seed + n, n_aircraft=max(1, min(40, n // 8)))
    items = []
    for j in range(len(base["frames"])):
        msg, rec = base["frames"]["bytes"][j].tobytes(), base["recs"][j]
        items.append((msg, int(rec["address"]), int(rec["kind"])))
        r = rng.random()
        if r < 0.15:
            items.append((other_frame(int(rec["address"])), int(rec["address"]), T.SELF))
        elif r < 0.25:
            items.append((msg, int(rec["address"]), T.UNKNOWN))
        elif r < 0.35:
            items.append((reply(CM.mb_17([7, int(rng.integers(8, 25))])), int(rec["address"]), T.KNOWN))
    return build(f"{n} frames", items[:n])


def claims_hold(case):
    claim = case["claim"]
    if claim is None:
        return
    out, records, table = run_model(case)
    if claim[0] == "mix":
        t = mix_tally(case, out)
        assert t[0x50]["right"] >= claim[1] // 20 and t[0x60]["right"] >= claim[1] // 200, t
        assert t[0x50]["wrong"] == 0 and t[0x60]["wrong"] == 0, t
    elif claim[0] == "frames":
        for j, (state, bds) in claim[1].items():
            assert (int(out["state"][j]), int(out["bds"][j])) == (state, bds), (case["name"], j, out[j])
    elif claim[0] == "counts":
        assert int(records["n_commb"].sum()) == claim[1] and int(records["n_ambiguous"].sum()) == claim[2], case["name"]
        assert int(records["n_settled"].sum()) == 0
    elif claim[0] == "stay":
        assert (out["state"][1:] == T.AMBIGUOUS).all() and len(out) > 2, case["name"]
        assert int(records["n_ambiguous"][0]) == len(out) - 1
    elif claim[0] == "registers":
        a = T.as_dict(records[list(sorted(table.state)).index(A)])
        assert a["capability"] and not math.isnan(a["ra_time"]) and a["n_none"] == 1 and a["n_ambiguous"] == 2
        assert all(not math.isnan(a[b]["time"]) for b in T.BLOCKS.values())
        assert (out[-2:].tobytes() == case["commb"][-2:].tobytes())
    else:
        raise AssertionError(claim[0])


def small_cases():
    return [registers(), twelve(), between(), no_commb(), none_ambiguous(), other_candidate_sets()] + \
           [boundary(v) for v in range(3)]
