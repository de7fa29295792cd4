"""The frame lists the extended squitter status stage is checked on (tests/test_es_host.py on the CPU mirror,
tests/test_gpu_es.py on the device), built with the model's ME makers.  Each case is (name, FRAME_DTYPE list, claim); the
claim is what the list is there to show, checked against the MODEL's records by claims_hold() so that a list cannot quietly
stop showing it:
  ("states", [state, ...])                     every frame's state
  ("fields", [{field: value, ...}, ...])       per frame: record fields by name, "has" / "lacks" lists of present names,
                                               "flags" the exact set of flag names, "half0" / "half1"
  None                                         nothing but model == library"""
import numpy as np

from tests import es_model as M

# frame (parity 0), then the fields the definition gives for it
KNOWN = (
    ("8DA2C1B6E112B600000000760759", dict(state=M.EMERGENCY, type_code=28, subtype=1, emergency=0, half0=6513,
                                          has=["EMERGENCY", "SQUAWK"])),
    ("8DA05629EA21485CBF3F8CADAEEB", dict(state=M.TARGET_STATE, type_code=29, subtype=1, version=2, value=16992, half0=10128,
                                          half1=95, nac_p=9, nic_baro=1, sil=3, sil_supplement=0,
                                          flags=["AUTOPILOT", "VNAV", "LNAV", "TCAS"],
                                          has=["SELECTED_ALT", "BARO", "HEADING", "MODES", "TCAS", "ALT_SOURCE", "VERSION"])),
    ("8D4840D6202CC371C32CE0576098", dict(state=M.CATEGORY, type_code=4, category=0xA0, has=["CATEGORY"])),
    ("8D485020994409940838175B284F", dict(state=M.VELOCITY, type_code=19, subtype=1, nac_v=0, flags=["IFR"],
                                          has=["NAC_V", "VELOCITY_FLAGS"])),
    ("8D40621D58C382D690C8AC2863A7", dict(state=M.POSITION, type_code=11, nic_b=0, value=1852, has=["NIC_B", "RC"])),
    ("8C4841753A9A153237AEF0F275BE", dict(state=M.POSITION, type_code=7, value=1852, has=["RC"], lacks=["NIC_B"])),
)
KNOWN_OPERATIONAL_ME = bytes.fromhex("F82300030049B8")
KNOWN_OPERATIONAL = dict(state=M.OPERATIONAL, type_code=31, subtype=0, version=2, half0=0x2300, half1=0x0300, nic_a=0, nac_p=9,
                         gva=2, sil=3, nic_baro=1, has=["VERSION", "CC_OM", "NIC_A", "NAC_P", "GVA", "SIL", "NIC_BARO", "SDA"])
KNOWN_FRAMES = [bytes.fromhex(k[0]) for k in KNOWN] + [M.frame(KNOWN_OPERATIONAL_ME)]
KNOWN_FIELDS = [k[1] for k in KNOWN] + [KNOWN_OPERATIONAL]
# a TC 29 payload with every optional value set, for the first-byte case
TARGET_FULL = M.me_target(alt=532, baro=267, heading=95, nac_p=9, nic_baro=1, sil=3, mode_status=1, modes=("AUTOPILOT", "LNAV"), tcas=1)
MODE_NAMES = ("AUTOPILOT", "VNAV", "ALT_HOLD", "APPROACH", "LNAV")


def known_answers():
    return "known answers", M.frame_list(KNOWN_FRAMES), ("fields", KNOWN_FIELDS)


def expected_state(tc, st):
    """the state table of the definition, spelt out row by row"""
    if 1 <= tc <= 4:
        return M.CATEGORY
    if tc == 0 or tc in range(5, 9) or tc in range(9, 19) or tc in range(20, 23):
        return M.POSITION
    if tc == 19:
        return M.VELOCITY if st in (1, 2, 3, 4) else M.RESERVED
    if tc == 28:
        return {1: M.EMERGENCY, 2: M.ACAS_RA}.get(st, M.RESERVED)
    if tc == 29:
        return M.TARGET_STATE if st >> 1 == 1 else M.RESERVED
    if tc == 31:
        return M.OPERATIONAL if st in (0, 1) else M.RESERVED
    return M.RESERVED                                               # TC 23-27, 30


def every_type_code_and_subtype():
    pairs = [(tc, st) for tc in range(32) for st in range(8)]
    msgs = [M.frame(M.me_tc(tc, st, rest=0x5A5A5A5A5A5A ^ (tc << 20 | st))) for tc, st in pairs]
    return "every TC x every subtype", M.frame_list(msgs), ("states", [expected_state(tc, st) for tc, st in pairs])


def every_first_byte():
    """every DF with every low three bits of byte 0 over a TC 29 payload: only DF 17 and DF 18 / CF 0, 1 are read"""
    msgs, states = [], []
    for df in range(32):
        for low3 in range(8):
            msgs.append(M.frame(TARGET_FULL, df=df, low3=low3))
            states.append(M.TARGET_STATE if df == 17 or (df == 18 and low3 in (0, 1)) else M.FOREIGN if df == 18 else M.NOT_ES)
    return "every first byte", M.frame_list(msgs), ("states", states)


def target_state_edges():
    rows = []
    for n, feet in ((0, None), (1, 0), (2047, 65472)):
        rows.append((M.me_target(alt=n), dict(value=feet or 0, **{"has" if n else "lacks": ["SELECTED_ALT"]})))
    for n, tenths in ((0, None), (1, 8000), (511, 12080)):
        rows.append((M.me_target(baro=n), dict(half0=tenths or 0, **{"has" if n else "lacks": ["BARO"]})))
    rows.append((M.me_target(heading=None, heading_raw=0x1FF), dict(half1=0, lacks=["HEADING"])))
    rows.append((M.me_target(heading=0x1FF), dict(half1=0x1FF, has=["HEADING"])))
    rows.append((M.me_target(heading=0), dict(half1=0, has=["HEADING"])))
    rows.append((M.me_target(mode_status=0, modes=MODE_NAMES, tcas=1), dict(flags=["TCAS"], lacks=["MODES"], has=["TCAS"])))
    rows.append((M.me_target(mode_status=1), dict(flags=[], has=["MODES", "TCAS", "ALT_SOURCE"])))
    for name in MODE_NAMES:
        rows.append((M.me_target(mode_status=1, modes=(name,)), dict(flags=[name], has=["MODES"])))
    rows.append((M.me_target(fms=1, sil_supp=1, nac_p=15, nic_baro=1, sil=3),
                 dict(flags=["ALT_FMS"], sil_supplement=1, nac_p=15, nic_baro=1, sil=3, version=2)))
    # the bits the definition leaves out (46, 51, 55, 56) change nothing
    rows.append((M.me_of({1: (5, 29), 6: (2, 1)}, ones=[46, 51, 55, 56]), dict(flags=[], lacks=["MODES", "SELECTED_ALT", "BARO", "HEADING"])))
    for r in rows:
        r[1].update(state=M.TARGET_STATE, type_code=29, subtype=1)
    return "TARGET_STATE edges", M.frame_list([M.frame(me) for me, _ in rows]), ("fields", [f for _, f in rows])


V2_ONLY, V12 = ["SIL_SUPPLEMENT", "SDA", "GVA", "NIC_C"], ["NIC_A", "NAC_P", "SIL", "HRD"]


def operational_versions():
    """versions 0..7 x ST 0, 1 over a payload with every bit behind the subtype set but the version's"""
    msgs, fields = [], []
    for version in range(8):
        for st in (0, 1):
            ones = (1 << 48) - 1 & ~(7 << 13) | version << 13     # u(41,3) is bits 15..13 of the 48 bits from bit 9
            msgs.append(M.frame(M.me_tc(31, st, rest=ones)))
            f = dict(state=M.OPERATIONAL, type_code=31, subtype=st, version=version, has=["VERSION"])
            if version == 0:
                f.update(has=["VERSION", "CC_OM"], lacks=V12 + V2_ONLY + ["NIC_BARO", "NAC_V", "LENGTH_WIDTH", "TRACK_HEADING"],
                         half0=0xFFFF, half1=0xFFFF)
            elif version in (1, 2):
                mine = ["NIC_BARO"] if st == 0 else ["TRACK_HEADING", "LENGTH_WIDTH"]
                other = ["TRACK_HEADING", "LENGTH_WIDTH"] if st == 0 else ["NIC_BARO"]
                v2 = ["SIL_SUPPLEMENT", "SDA"] + (["GVA"] if st == 0 else ["NIC_C", "NAC_V"])
                f.update(has=["VERSION", "CC_OM"] + V12 + mine + (v2 if version == 2 else []),
                         lacks=other + (V2_ONLY + ["NAC_V"] if version == 1 else ["NIC_C", "NAC_V"] if st == 0 else ["GVA"]),
                         nic_a=1, nac_p=15, sil=3, flags=["HRD"] + (["TRACK_HEADING"] if st else []))
                if version == 2:
                    f.update(sil_supplement=1, sda=3, **(dict(gva=3, nic_c=0, nac_v=0) if st == 0 else dict(gva=0, nic_c=1, nac_v=7)))
                else:
                    f.update(sil_supplement=0, sda=0, gva=0, nic_c=0, nac_v=0)
                f.update(dict(nic_baro=1, length_width=0) if st == 0 else dict(nic_baro=0, length_width=15))
            else:
                f.update(lacks=["CC_OM"] + V12 + V2_ONLY + ["NIC_BARO", "NAC_V"], half0=0, half1=0, nac_p=0, sil=0, flags=[])
            fields.append(f)
    return "OPERATIONAL: versions 0..7 x ST 0, 1", M.frame_list(msgs), ("fields", fields)


def emergency_states():
    msgs = [M.frame(M.me_emergency(state=s, code=(7500, 7600, 7700, 1234, 0, 7777, 4321, 2000)[s])) for s in range(8)]
    fields = [dict(state=M.EMERGENCY, emergency=s, half0=(7500, 7600, 7700, 1234, 0, 7777, 4321, 2000)[s]) for s in range(8)]
    return "EMERGENCY: all eight states", M.frame_list(msgs), ("fields", fields)


def every_squawk():
    """all 4096 squawks, each with X clear and X set"""
    codes = [int(f"{k:04o}") for k in range(4096)]
    msgs = [M.frame(M.me_emergency(state=k & 7, code=c, x=x)) for k, c in enumerate(codes) for x in (0, 1)]
    fields = [dict(state=M.EMERGENCY, half0=c, emergency=k & 7) for k, c in enumerate(codes) for x in (0, 1)]
    return "EMERGENCY: all 4096 squawks, X clear and set", M.frame_list(msgs), ("fields", fields)


def acas_ra_walking_one():
    msgs = [M.frame(M.me_tc(28, 2, rest=1 << k)) for k in range(47, -1, -1)] + [M.frame(M.me_tc(28, 2)), M.frame(M.me_tc(28, 2, (1 << 48) - 1))]
    fields = [dict(state=M.ACAS_RA, subtype=2, value=(1 << k) >> 16, half0=(1 << k) & 0xFFFF, has=["RA"]) for k in range(47, -1, -1)]
    fields += [dict(state=M.ACAS_RA, value=0, half0=0, has=["RA"]), dict(state=M.ACAS_RA, value=0xFFFFFFFF, half0=0xFFFF, half1=0)]
    return "ACAS_RA: a walking one over the 48 bits", M.frame_list(msgs), ("fields", fields)


def positions_and_velocities():
    """every position type code with bit 8 set: nic_b on TC 9-18 only, Rc by the version-0 column; the velocity bits"""
    rc = {0: 0, 5: 75, 6: 250, 7: 1852, 8: 0, 9: 75, 10: 250, 11: 1852, 12: 3704, 13: 9260, 14: 18520, 15: 37040, 16: 185200,
          17: 370400, 18: 0, 20: 75, 21: 250, 22: 0}
    msgs, fields = [], []
    for tc, dm in rc.items():
        msgs.append(M.frame(M.me_tc(tc, st=1, rest=0x123456789ABC)))
        holds = {"NIC_B": 9 <= tc <= 18, "RC": dm != 0}
        fields.append(dict(state=M.POSITION, type_code=tc, subtype=0, value=dm, nic_b=int(holds["NIC_B"]),
                           has=[k for k, on in holds.items() if on], lacks=[k for k, on in holds.items() if not on]))
    for st in (1, 2, 3, 4):
        for intent, ifr, nac_v in ((0, 0, 0), (1, 0, 7), (0, 1, 5), (1, 1, 2)):
            msgs.append(M.frame(M.me_of({1: (5, 19), 6: (3, st), 9: (1, intent), 10: (1, ifr), 11: (3, nac_v), 14: (43, 0x2AAAAAAAAAA)})))
            fields.append(dict(state=M.VELOCITY, subtype=st, nac_v=nac_v, has=["NAC_V", "VELOCITY_FLAGS"],
                               flags=[n for n, on in (("INTENT_CHANGE", intent), ("IFR", ifr)) if on]))
    for tc in (1, 2, 3, 4):
        for ca in (0, 7):
            msgs.append(M.frame(M.me_tc(tc, st=ca, rest=0x0C3071C32CE0)))
            fields.append(dict(state=M.CATEGORY, type_code=tc, subtype=0, category=int({4: "A", 3: "B", 2: "C", 1: "D"}[tc], 16) << 4 | ca))
    return "positions, velocities and categories", M.frame_list(msgs), ("fields", fields)


def short_frames():
    """wire input's short frames: bytes[7..14) = 0, every short format"""
    msgs = [bytes([df << 3 | low3, 0x12, 0x34, 0x56, 0xE9, 0x21, 0x48]) for df in range(16) for low3 in (0, 5)]
    return "short frames", M.frame_list(msgs), ("states", [M.NOT_ES] * len(msgs))


def claims_hold(case):
    """the claim of a case against the model's records"""
    name, fr, claim = case
    recs = M.es(fr)["recs"]
    if claim is None:
        return
    assert len(recs) == len(claim[1]), name
    if claim[0] == "states":
        assert recs["state"].tolist() == claim[1], name
        return
    assert claim[0] == "fields"
    for j, (r, want) in enumerate(zip(recs, claim[1])):
        for key, v in want.items():
            if key == "has":
                assert all(int(r["present"]) & M.HAS[k] for k in v), (name, j, key, v, r)
            elif key == "lacks":
                assert not any(int(r["present"]) & M.HAS[k] for k in v), (name, j, key, v, r)
            elif key == "flags":
                assert int(r["flags"]) == sum(M.FLAG[k] for k in v), (name, j, key, v, r)
            elif key in ("half0", "half1"):
                assert int(r["half"][int(key[-1])]) == v, (name, j, key, v, r)
            else:
                assert int(r[key]) == v, (name, j, key, v, r)


# ---- a long mixed list ---------------------------------------------------------------------------------------------------
def random_list(n, seed):
    """n frames: half of them uniformly random bytes, the rest DF17 / DF18 frames of a random type code with random ME
    bits, a share of them steered to the states random bits rarely reach (TC 28 ST 1 / 2, TC 29 subtype 1, TC 31 ST 0 / 1
    with versions 0..3)"""
    rng = np.random.default_rng(seed)
    fr = np.zeros(n, dtype=M.FRAME_DTYPE)
    b = rng.integers(0, 256, size=(n, 14)).astype(np.uint8)
    built = np.flatnonzero(rng.integers(0, 2, size=n) == 1)
    sort = rng.integers(0, 8, size=len(built))
    df18 = rng.integers(0, 4, size=len(built)) == 0
    b[built, 0] = np.where(df18, 18 << 3 | rng.integers(0, 3, size=len(built)), 17 << 3 | rng.integers(0, 8, size=len(built))).astype(np.uint8)
    b4 = b[built, 4]
    b4 = np.where(sort == 1, 28 << 3 | rng.integers(1, 3, size=len(built)), b4)
    b4 = np.where(sort == 2, 29 << 3 | 2 | (b4 & 1), b4)
    b4 = np.where(sort == 3, 31 << 3 | rng.integers(0, 2, size=len(built)), b4)
    b4 = np.where(sort == 4, 19 << 3 | rng.integers(0, 8, size=len(built)), b4)
    b[built, 4] = b4.astype(np.uint8)
    steer = built[sort == 3]                                        # versions 0..3 as often as each other: u(41,3) is the top of bytes[9]
    b[steer, 9] = (b[steer, 9] & 0x1F) | (rng.integers(0, 4, size=len(steer)) << 5).astype(np.uint8)
    fr["bytes"], fr["offset"], fr["fixed_bit"] = b, np.arange(n) * 240, 0xFF
    return fr


def covers_everything(recs):
    """every state and every version total are in these records"""
    assert set(recs["state"].tolist()) == set(range(10))
    assert set(np.minimum(recs["version"][recs["state"] == M.OPERATIONAL], 3).tolist()) == {0, 1, 2, 3}


def all_cases():
    return [known_answers(), every_type_code_and_subtype(), every_first_byte(), target_state_edges(), operational_versions(),
            emergency_states(), every_squawk(), acas_ra_walking_one(), positions_and_velocities(), short_frames(),
            ("a random list", random_list(400, 7), None)]
