"""Independent model of the extended squitter status stage (include/adsb_hip.h, "Extended squitter status"), written from
the definition in plain Python: ME as a string of 56 binary digits, so that bit a of the text is character a - 1, the
state rules in their order, the fields state by state, and the integrity table as a table.  Calls no library entry point.
Shared by the CPU and GPU tiers, with the comparison of a library result against it and the makers of valid DF17 frames
(parity computed) the case lists are built with."""
import numpy as np

from tests import modes_model as S

(NOT_ES, FOREIGN, CATEGORY, POSITION, VELOCITY, EMERGENCY, ACAS_RA, TARGET_STATE, OPERATIONAL, RESERVED) = range(10)
STATE_NAMES = ("NOT_ES", "FOREIGN", "CATEGORY", "POSITION", "VELOCITY", "EMERGENCY", "ACAS_RA", "TARGET_STATE", "OPERATIONAL",
               "RESERVED")
PRESENT_NAMES = ("CATEGORY", "NIC_B", "RC", "NAC_V", "VELOCITY_FLAGS", "EMERGENCY", "SQUAWK", "RA", "SIL_SUPPLEMENT",
                 "ALT_SOURCE", "SELECTED_ALT", "BARO", "HEADING", "NAC_P", "NIC_BARO", "SIL", "MODES", "TCAS", "VERSION", "CC_OM",
                 "NIC_A", "HRD", "TRACK_HEADING", "LENGTH_WIDTH", "SDA", "GVA", "NIC_C")
HAS = {name: 1 << k for k, name in enumerate(PRESENT_NAMES)}
FLAG_NAMES = ("INTENT_CHANGE", "IFR", "ALT_FMS", "AUTOPILOT", "VNAV", "ALT_HOLD", "APPROACH", "LNAV", "TCAS", "HRD", "TRACK_HEADING")
FLAG = {name: 1 << k for k, name in enumerate(FLAG_NAMES)}
VERSION_UNKNOWN = 0xFF
BYTE_FIELDS = ("nic_a", "nic_b", "nic_c", "nac_p", "nac_v", "sil", "sil_supplement", "gva", "sda", "nic_baro", "category",
               "emergency", "length_width", "reserved")
FRAME_DTYPE = np.dtype([("offset", "<u8"), ("bytes", "u1", (14,)), ("status", "u1"), ("fixed_bit", "u1")])
REC_DTYPE = np.dtype([("state", "u1"), ("type_code", "u1"), ("subtype", "u1"), ("version", "u1"), ("present", "<u4")]
                     + [(k, "u1") for k in BYTE_FIELDS] + [("flags", "<u2"), ("value", "<u4"), ("half", "<u2", (2,))])
HEADER_DTYPE = np.dtype([("n", "<u8"), ("n_state", "<u8", (10,)), ("n_version", "<u8", (4,)), ("reserved", "<u8")])

# the integrity table: Rc in decimetres by its value in metres as the definition prints it
DM = {"7.5": 75, "25": 250, "75": 750, "185.2": 1852, "370.4": 3704, "555.6": 5556, "926": 9260, "1111.2": 11112, "1852": 18520,
      "3704": 37040, "7408": 74080, "14816": 148160, "18520": 185200, "37040": 370400, "-": 0}


def integrity(tc, version, supp):
    """(NIC, Rc in dm) by the table of the definition; supp: bit 0 = A, bit 1 = B, bit 2 = C"""
    v = 0 if version == VERSION_UNKNOWN else min(version, 2)
    A, B, Cc = bool(supp & 1), bool(supp & 2), bool(supp & 4)
    v0 = {0: "-", 18: "-", 22: "-", 9: "7.5", 20: "7.5", 10: "25", 21: "25", 11: "185.2", 12: "370.4", 13: "926", 14: "1852",
          15: "3704", 16: "18520", 17: "37040", 5: "7.5", 6: "25", 7: "185.2", 8: "-"}
    if tc not in v0:
        return 0, 0
    if v == 0:
        return 0, DM[v0[tc]]
    fixed = {0: (0, "-"), 18: (0, "-"), 22: (0, "-"), 9: (11, "7.5"), 20: (11, "7.5"), 10: (10, "25"), 21: (10, "25"),
             12: (7, "370.4"), 14: (5, "1852"), 15: (4, "3704"), 17: (1, "37040"), 5: (11, "7.5"), 6: (10, "25")}
    if tc in fixed:
        nic, rc = fixed[tc]
    elif tc == 11:
        nic, rc = (9, "75") if (A if v == 1 else A and B) else (8, "185.2")
    elif tc == 13:
        if v == 1:
            nic, rc = 6, "1111.2" if A else "926"
        else:
            nic, rc = 6, {(True, True): "1111.2", (False, True): "555.6", (False, False): "926", (True, False): "1111.2"}[(A, B)]
    elif tc == 16:
        nic, rc = (3, "7408") if (A if v == 1 else A and B) else (2, "14816")
    elif tc == 7:
        nic, rc = (9, "75") if (A if v == 1 else A and not Cc) else (8, "185.2")
    else:
        assert tc == 8
        if v == 1:
            nic, rc = 0, "-"
        else:
            nic, rc = {(True, True): (7, "370.4"), (True, False): (6, "555.6"), (False, True): (6, "1111.2"),
                       (False, False): (0, "-")}[(A, Cc)]
    return nic, DM[rc]


class ME:
    """the 56 bits, numbered from 1"""

    def __init__(self, seven_bytes):
        assert len(seven_bytes) == 7
        self.digits = "".join(f"{x:08b}" for x in bytes(seven_bytes))

    def u(self, a, n):
        assert 1 <= a and a + n - 1 <= 56
        return int(self.digits[a - 1:a - 1 + n], 2)


def squawk_of(m, a):
    """the 13 bits from bit a, C1 A1 C2 A2 C4 A4 X B1 D1 B2 D2 B4 D4, as four octal digits read in decimal"""
    bit = dict(zip("C1 A1 C2 A2 C4 A4 X B1 D1 B2 D2 B4 D4".split(), (int(ch) for ch in m.digits[a - 1:a + 12])))
    digit = lambda g: 4 * bit[g + "4"] + 2 * bit[g + "2"] + bit[g + "1"]
    return 1000 * digit("A") + 100 * digit("B") + 10 * digit("C") + digit("D")


def state_of(df, low3, m):
    """(state, type code, subtype) by the first rule that applies"""
    if df not in (17, 18):
        return NOT_ES, 0, 0
    if df == 18 and low3 not in (0, 1):
        return FOREIGN, 0, 0
    tc, st = m.u(1, 5), m.u(6, 3)
    if 1 <= tc <= 4:
        return CATEGORY, tc, 0
    if tc == 0 or 5 <= tc <= 18 or 20 <= tc <= 22:
        return POSITION, tc, 0
    if tc == 19 and 1 <= st <= 4:
        return VELOCITY, tc, st
    if tc == 28 and st == 1:
        return EMERGENCY, tc, st
    if tc == 28 and st == 2:
        return ACAS_RA, tc, st
    if tc == 29:
        return (TARGET_STATE if m.u(6, 2) == 1 else RESERVED), tc, m.u(6, 2)
    if tc == 31 and st <= 1:
        return OPERATIONAL, tc, st
    return RESERVED, tc, st


def fields_of(state, tc, st, m):
    """{field: value} of what the record holds beside state, type_code and subtype, and the set of present names.  flags
    as a set of names; value, half0, half1 as the numbers"""
    f, has, flags = {}, set(), set()

    def put(name, field, value):
        f[field] = value
        has.add(name)

    def flag(name, on):
        if on:
            flags.add(name)

    if state == CATEGORY:
        put("CATEGORY", "category", (0xE - tc) << 4 | m.u(6, 3))
    elif state == POSITION:
        if 9 <= tc <= 18:
            put("NIC_B", "nic_b", m.u(8, 1))
        rc = integrity(tc, 0, 0)[1]
        if rc:
            put("RC", "value", rc)
    elif state == VELOCITY:
        put("NAC_V", "nac_v", m.u(11, 3))
        has.add("VELOCITY_FLAGS")
        flag("INTENT_CHANGE", m.u(9, 1))
        flag("IFR", m.u(10, 1))
    elif state == EMERGENCY:
        put("EMERGENCY", "emergency", m.u(9, 3))
        put("SQUAWK", "half0", squawk_of(m, 12))
    elif state == ACAS_RA:
        has.add("RA")
        f["value"], f["half0"] = m.u(9, 32), m.u(41, 16)
    elif state == TARGET_STATE:
        put("VERSION", "version", 2)
        put("SIL_SUPPLEMENT", "sil_supplement", m.u(8, 1))
        has.add("ALT_SOURCE")
        flag("ALT_FMS", m.u(9, 1))
        if m.u(10, 11):
            put("SELECTED_ALT", "value", 32 * (m.u(10, 11) - 1))
        if m.u(21, 9):
            put("BARO", "half0", 8000 + 8 * (m.u(21, 9) - 1))
        if m.u(30, 1):
            put("HEADING", "half1", m.u(31, 9))
        put("NAC_P", "nac_p", m.u(40, 4))
        put("NIC_BARO", "nic_baro", m.u(44, 1))
        put("SIL", "sil", m.u(45, 2))
        if m.u(47, 1):
            has.add("MODES")
            for name, a in (("AUTOPILOT", 48), ("VNAV", 49), ("ALT_HOLD", 50), ("APPROACH", 52), ("LNAV", 54)):
                flag(name, m.u(a, 1))
        has.add("TCAS")
        flag("TCAS", m.u(53, 1))
    elif state == OPERATIONAL:
        version = m.u(41, 3)
        put("VERSION", "version", version)
        if version <= 2:
            has.add("CC_OM")
            f["half0"], f["half1"] = m.u(9, 16), m.u(25, 16)
        if version in (1, 2):
            put("NIC_A", "nic_a", m.u(44, 1))
            put("NAC_P", "nac_p", m.u(45, 4))
            put("SIL", "sil", m.u(51, 2))
            has.add("HRD")
            flag("HRD", m.u(54, 1))
            if st == 0:
                put("NIC_BARO", "nic_baro", m.u(53, 1))
            else:
                has.add("TRACK_HEADING")
                flag("TRACK_HEADING", m.u(53, 1))
                put("LENGTH_WIDTH", "length_width", m.u(21, 4))
        if version == 2:
            put("SIL_SUPPLEMENT", "sil_supplement", m.u(55, 1))
            put("SDA", "sda", m.u(31, 2))
            if st == 0:
                put("GVA", "gva", m.u(49, 2))
            else:
                put("NIC_C", "nic_c", m.u(20, 1))
                put("NAC_V", "nac_v", m.u(17, 3))
    return f, has, flags


NOTHING = (0, 0, 0, 0, 0) + (0,) * len(BYTE_FIELDS) + (0, 0, [0, 0])


def record(frame_bytes):
    """One frame's record as a REC_DTYPE scalar's tuple."""
    b = bytes(frame_bytes)
    df, low3 = b[0] >> 3, b[0] & 7
    if df not in (17, 18):
        return NOTHING
    m = ME(b[4:11])
    state, tc, st = state_of(df, low3, m)
    if state == FOREIGN:
        return (FOREIGN,) + NOTHING[1:]
    f, has, flags = fields_of(state, tc, st, m)
    return ((state, tc, st, f.get("version", 0), sum(HAS[k] for k in has)) + tuple(f.get(k, 0) for k in BYTE_FIELDS)
            + (sum(FLAG[k] for k in flags), f.get("value", 0), [f.get("half0", 0), f.get("half1", 0)]))


def es(frames):
    """The whole definition over a FRAME_DTYPE array (or a list of 14-byte strings) -> dict(recs, header)."""
    if not isinstance(frames, np.ndarray):
        frames = frame_list(frames)
    recs = np.zeros(len(frames), dtype=REC_DTYPE)
    df = frames["bytes"][:, 0] >> 3
    for j in np.flatnonzero((df == 17) | (df == 18)):                # every other record is all zero
        recs[j] = record(frames["bytes"][j].tobytes())
    operational = recs["state"] == OPERATIONAL
    header = dict(n=len(frames), n_state=[int((recs["state"] == s).sum()) for s in range(10)],
                  n_version=[int((operational & (recs["version"] == v)).sum()) for v in (0, 1, 2)]
                  + [int((operational & (recs["version"] >= 3)).sum())], reserved=0)
    return dict(recs=recs, header=header)


def header_dict(header):
    """a library header (ES_HEADER_DTYPE record) as the model spells it"""
    return dict(n=int(header["n"]), n_state=[int(x) for x in header["n_state"]], n_version=[int(x) for x in header["n_version"]],
                reserved=int(header["reserved"]))


def same(got, want, what=""):
    """A library result (recs, header) against the model's, byte for byte."""
    recs, header = got
    assert header_dict(header) == want["header"], (what, header, want["header"])
    assert len(recs) == len(want["recs"]), (what, len(recs), len(want["recs"]))
    if recs.tobytes() != want["recs"].tobytes():
        bad = [j for j in range(len(recs)) if recs[j].tobytes() != want["recs"][j].tobytes()][:4]
        raise AssertionError((what, "recs", [(j, recs[j], want["recs"][j]) for j in bad]))


# ---- frames and ME fields ------------------------------------------------------------------------------------------------
def frame_list(msgs):
    fr = np.zeros(len(msgs), dtype=FRAME_DTYPE)
    for i, msg in enumerate(msgs):
        fr["bytes"][i][:len(msg)] = np.frombuffer(bytes(msg), dtype=np.uint8)
    fr["offset"] = np.arange(len(msgs)) * 500
    fr["fixed_bit"] = 0xFF
    return fr


def frame(me, df=17, low3=5, aa=0x4840D6):
    """A 14-byte frame of format df around the 7 bytes of me, with the parity that makes its syndrome 0 (for DF17/18: a
    valid extended squitter; for an address/parity format: a reply from address 0)."""
    assert len(me) == 7
    head = bytes([df << 3 | low3]) + aa.to_bytes(3, "big") + bytes(me)
    return head + S.crc24(head).to_bytes(3, "big")


def me_of(fields, ones=()):
    """ME from {first bit: (width, value)} and single bits set."""
    v = 0
    for a, (n, x) in fields.items():
        assert 0 <= x < (1 << n) and a + n - 1 <= 56
        v |= x << (57 - a - n)
    for a in ones:
        v |= 1 << (56 - a)
    return v.to_bytes(7, "big")


def me_tc(tc, st=0, rest=0):
    """type code, u(6,3) and the 48 bits behind them as a number"""
    return me_of({1: (5, tc), 6: (3, st), 9: (48, rest)})


def squawk_bits(code):
    """the 13 bits (X = 0) of a squawk given as four octal digits read in decimal"""
    d = {g: code // 10 ** k % 10 for g, k in zip("ABCD", (3, 2, 1, 0))}
    names = "C1 A1 C2 A2 C4 A4 X B1 D1 B2 D2 B4 D4".split()
    return int("".join("0" if n == "X" else str(d[n[0]] >> {"1": 0, "2": 1, "4": 2}[n[1]] & 1) for n in names), 2)


def me_emergency(state=0, code=0, x=0):
    return me_of({1: (5, 28), 6: (3, 1), 9: (3, state), 12: (13, squawk_bits(code) | x << 6)})


def me_target(alt=0, baro=0, heading=None, fms=0, sil_supp=0, nac_p=0, nic_baro=0, sil=0, mode_status=0, modes=(), tcas=0,
              heading_raw=0):
    """TC 29 subtype 1.  alt, baro: the raw n; heading: the raw 9 bits with the status bit set (None: status off over
    heading_raw); modes: names among AUTOPILOT VNAV ALT_HOLD APPROACH LNAV, set whatever mode_status says"""
    at = dict(AUTOPILOT=48, VNAV=49, ALT_HOLD=50, APPROACH=52, LNAV=54)
    f = {1: (5, 29), 6: (2, 1), 8: (1, sil_supp), 9: (1, fms), 10: (11, alt), 21: (9, baro),
         30: (1, 0 if heading is None else 1), 31: (9, heading_raw if heading is None else heading), 40: (4, nac_p),
         44: (1, nic_baro), 45: (2, sil), 47: (1, mode_status), 53: (1, tcas)}
    return me_of(f, ones=[at[k] for k in modes])


def me_operational(st=0, version=2, cc=0, om=0, nic_a=0, nac_p=0, gva_or_rest=0, sil=0, bit53=0, hrd=0, sil_supp=0):
    """TC 31; gva_or_rest: u(49,2)"""
    return me_of({1: (5, 31), 6: (3, st), 9: (16, cc), 25: (16, om), 41: (3, version), 44: (1, nic_a), 45: (4, nac_p),
                  49: (2, gva_or_rest), 51: (2, sil), 53: (1, bit53), 54: (1, hrd), 55: (1, sil_supp)})
