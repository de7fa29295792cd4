"""Independent model of the Mode S stage (include/adsb_hip.h, "Mode S replies"), written from the definitions in plain
Python and NumPy: CRC-24 by bitwise long division, the kinds, the causal known rule with a dict, the AC field (25 ft and
Gillham, the steps written out over named bits), the ID field, the flags and the BDS 2,0 callsign.  Calls no library
entry point.  Shared by the CPU and GPU tiers, with the comparison of a library result against it."""
import numpy as np

GENERATOR = 0x1FFF409
SELF, KNOWN, UNKNOWN, PARITY, UNSUPPORTED = range(5)
KIND_NAMES = ("SELF", "KNOWN", "UNKNOWN", "PARITY", "UNSUPPORTED")
ALT, ALT_METRIC, SQUAWK, GROUND, ALERT, SPI, CALLSIGN = 1, 2, 4, 8, 16, 32, 64
ALL_FLAGS = (ALT, ALT_METRIC, SQUAWK, GROUND, ALERT, SPI, CALLSIGN)
ADDRESS_PARITY = (0, 4, 5, 16, 20, 21) + tuple(range(24, 32))
SELF_CHECKING = (11, 17, 18)
SUPPORTED = ADDRESS_PARITY + SELF_CHECKING
CHARSET = "#ABCDEFGHIJKLMNOPQRSTUVWXYZ#####_###############0123456789######"
HEADER_FIELDS = ("n", "n_self", "n_known", "n_unknown", "n_parity", "n_unsupported", "n_known_out", "n_squitters")
FRAME_DTYPE = np.dtype([("offset", "<u8"), ("bytes", "u1", (14,)), ("status", "u1"), ("fixed_bit", "u1")])
REC_DTYPE = np.dtype([("address", "<u4"), ("df", "u1"), ("kind", "u1"), ("flags", "<u2"), ("altitude_ft", "<i4"),
                      ("squawk", "<u2"), ("fs", "u1"), ("dr", "u1"), ("um", "u1"), ("iid", "u1"), ("ca", "u1"), ("ri", "u1"),
                      ("callsign", "S8"), ("reserved", "u1", (4,))])
# the 13-bit field, bit 12 down to bit 0
NAMES = ("C1", "A1", "C2", "A2", "C4", "A4", "M", "B1", "Q", "B2", "D2", "B4", "D4")


def crc24(data):
    """The remainder of data x 2^24 divided by the generator, by long division over a Python integer."""
    v = int.from_bytes(bytes(data), "big") << 24
    for i in range(v.bit_length() - 1, 23, -1):
        if v >> i & 1:
            v ^= GENERATOR << (i - 24)
    return v


def crc24_many(rows):
    """crc24 of every row of a uint8 array [n, k]: the same division, one message bit of every row at a time."""
    rows = np.asarray(rows, dtype=np.uint8)
    r = np.zeros(len(rows), dtype=np.uint32)
    for b in range(rows.shape[1]):
        for i in range(7, -1, -1):
            feed = ((r >> 23) & 1) ^ ((rows[:, b] >> i) & 1)
            r = ((r << 1) & 0xFFFFFF) ^ (feed * np.uint32(GENERATOR & 0xFFFFFF))
    return r


def length(df):
    return 7 if df < 16 else 14


def syndrome(b):
    n = length(b[0] >> 3)
    return crc24(b[:n - 3]) ^ int.from_bytes(bytes(b[n - 3:n]), "big")


def bits_of(f):
    """The 13-bit field as a dict of its named bits."""
    return {name: f >> (12 - k) & 1 for k, name in enumerate(NAMES)}


def field_of(**bits):
    """The 13-bit field with the named bits set (Q and D1 are the same bit, as are M and the ID field's zero)."""
    f = 0
    for name, v in bits.items():
        name = {"D1": "Q"}.get(name, name)
        f |= (1 if v else 0) << (12 - NAMES.index(name))
    return f


def gray_to_binary(bits):
    """Bits of a Gray code, most significant first -> its number: every binary bit is the XOR of the Gray bits above and at it."""
    value, acc = 0, 0
    for g in bits:
        acc ^= g
        value = value << 1 | acc
    return value


def gillham(f):
    """A Gillham-coded AC field (M = Q = 0) -> feet, or None for a code that stands for no altitude."""
    x = bits_of(f)
    h = gray_to_binary([x["D2"], x["D4"], x["A1"], x["A2"], x["A4"], x["B1"], x["B2"], x["B4"]])      # 500 ft steps
    c = gray_to_binary([x["C1"], x["C2"], x["C4"]])                                                   # 100 ft steps
    c = {5: 7, 7: 5}.get(c, c)
    if c == 0 or c > 5:
        return None
    if h % 2:
        c = 6 - c                                                   # the 100 ft steps run back in every odd 500 ft step
    return 500 * h + 100 * c - 1300


def altitude(f):
    """The AC field -> (flags, feet)."""
    if f == 0:
        return 0, 0
    x = bits_of(f)
    if x["M"]:
        return ALT_METRIC, 0
    if x["Q"]:
        n = 0
        for name in ("C1", "A1", "C2", "A2", "C4", "A4", "B1", "B2", "D2", "B4", "D4"):       # the field without M and Q
            n = n << 1 | x[name]
        return ALT, 25 * n - 1000
    feet = gillham(f)
    return (0, 0) if feet is None else (ALT, feet)


def squawk(f):
    x = bits_of(f)
    x["D1"] = x["Q"]
    digit = lambda l: 4 * x[l + "4"] + 2 * x[l + "2"] + x[l + "1"]
    return 1000 * digit("A") + 100 * digit("B") + 10 * digit("C") + digit("D")


def first_pass(b):
    """One frame's record as a dict, with kind None where the known set decides between KNOWN and UNKNOWN."""
    b = bytes(b)
    df = b[0] >> 3
    r = dict(address=0, df=df, kind=UNSUPPORTED, flags=0, altitude_ft=0, squawk=0, fs=0, dr=0, um=0, iid=0, ca=0, ri=0,
             callsign=b"")
    if df not in SUPPORTED:
        return r
    s, aa = syndrome(b), int.from_bytes(b[1:4], "big")
    if df in ADDRESS_PARITY:
        r["kind"], r["address"] = None, s
    elif s == 0:
        r["kind"], r["address"] = SELF, aa
    elif df == 11 and s < 0x80:
        r["kind"], r["address"], r["iid"] = None, aa, s
    else:
        r["kind"] = PARITY
    if df in SELF_CHECKING:
        r["ca"] = b[0] & 7
    f = (b[2] & 0x1F) << 8 | b[3]
    if df in (4, 5, 20, 21):
        fs = r["fs"] = b[0] & 7
        r["dr"], r["um"] = b[1] >> 3, (b[1] & 7) << 3 | b[2] >> 5
        r["flags"] |= (GROUND if fs in (1, 3) else 0) | (ALERT if fs in (2, 3, 4) else 0) | (SPI if fs in (4, 5) else 0)
    if df in (0, 16):
        r["flags"] |= GROUND if b[0] >> 2 & 1 else 0
        r["ri"] = (b[1] & 7) << 1 | b[2] >> 7
    if df in (0, 4, 16, 20):
        flags, r["altitude_ft"] = altitude(f)
        r["flags"] |= flags
    if df in (5, 21):
        r["squawk"], r["flags"] = squawk(f), r["flags"] | SQUAWK
    if df in (20, 21) and b[4] == 0x20:
        v = int.from_bytes(b[5:11], "big")
        text = "".join(CHARSET[v >> (42 - 6 * k) & 0x3F] for k in range(8))
        r["callsign"] = text.encode()
        if "#" not in text:
            r["flags"] |= CALLSIGN
    return r


def modes(frames, known_in=(), counts=None):
    """The whole definition over a FRAME_DTYPE array (or a list of 14-byte strings) -> dict(recs, known_out, squitters,
    squitter_counts, header).  The known rule is a dict from address to the list index from which it is known."""
    if not isinstance(frames, np.ndarray):
        frames = frame_list(frames)
    since = {int(a): 0 for a in known_in}
    recs = np.zeros(len(frames), dtype=REC_DTYPE)
    squitter = []
    for j, row in enumerate(frames["bytes"]):
        r = first_pass(row.tobytes())
        if r["kind"] is None:
            r["kind"] = KNOWN if since.get(r["address"], j + 1) <= j else UNKNOWN
        if r["kind"] == SELF:
            since.setdefault(r["address"], j + 1)
            if r["df"] in (17, 18):
                squitter.append(j)
        recs[j] = tuple(r[k] for k in REC_DTYPE.names[:-1]) + ([0, 0, 0, 0],)
    header = dict(n=len(frames), n_known_out=len(since), n_squitters=len(squitter))
    for k, name in enumerate(KIND_NAMES):
        header["n_" + name.lower()] = int((recs["kind"] == k).sum())
    sq_counts = None
    if counts is not None:
        edges = np.cumsum([0] + [int(c) for c in counts])
        assert edges[-1] == len(frames)
        at = np.array(squitter, dtype=np.int64)
        sq_counts = np.array([((at >= a) & (at < b)).sum() for a, b in zip(edges, edges[1:])], dtype=np.uint64)
    return dict(recs=recs, known_out=np.array(sorted(since), dtype=np.uint32), squitters=frames[squitter].copy(),
                squitter_counts=sq_counts, header=header)


def same(got, want, what=""):
    """A library result (recs, known_out, squitters, squitter_counts, header) against the model's, byte for byte."""
    recs, known_out, squitters, sq_counts, header = got
    assert {k: int(header[k]) for k in HEADER_FIELDS} == want["header"], (what, header, want["header"])
    if recs.tobytes() != want["recs"].tobytes():
        bad = [j for j in range(len(recs)) if recs[j].tobytes() != want["recs"][j].tobytes()][:4]
        raise AssertionError((what, "recs", [(j, recs[j], want["recs"][j]) for j in bad]))
    assert known_out.tolist() == want["known_out"].tolist(), (what, "known_out")
    assert squitters.tobytes() == want["squitters"].tobytes(), (what, "squitters")
    assert (sq_counts is None) == (want["squitter_counts"] is None), what
    if sq_counts is not None:
        assert sq_counts.tolist() == want["squitter_counts"].tolist(), (what, "squitter_counts")


# ---- frames --------------------------------------------------------------------------------------------------------------
def frame_list(msgs, offsets=None):
    """7- or 14-byte messages -> a FRAME_DTYPE list (short ones padded with zeros, as wire input emits them)."""
    fr = np.zeros(len(msgs), dtype=FRAME_DTYPE)
    for i, m in enumerate(msgs):
        fr["bytes"][i][:len(m)] = np.frombuffer(bytes(m), dtype=np.uint8)
    fr["offset"] = np.arange(len(msgs)) * 500 if offsets is None else offsets
    fr["fixed_bit"] = 0xFF
    return fr


def overlay(payload, word):
    """payload + (crc24(payload) ^ word): word = 0 a self-checking frame, an address an address/parity reply, an iid
    DF11's reply to that interrogator."""
    return bytes(payload) + (crc24(payload) ^ word).to_bytes(3, "big")


def reply(df, address, low3=0, b1=0, b2_high=0, field=0, rest=bytes(7)):
    """An address/parity reply: byte 0 = df and its three low bits (FS, or VS and two more), byte 1, the 13-bit field in
    bytes 2-3 under byte 2's three high bits, for a long DF the 7 bytes of MB / MV."""
    head = bytes([df << 3 | low3, b1 & 0xFF, (b2_high & 7) << 5 | field >> 8, field & 0xFF])
    return overlay(head + (bytes(rest) if df >= 16 else b""), address)


def all_call(aa, iid=0, ca=5):
    return overlay(bytes([11 << 3 | ca]) + aa.to_bytes(3, "big"), iid)


def squitter(aa, df=17, ca=5, me=bytes(7)):
    return overlay(bytes([df << 3 | ca]) + aa.to_bytes(3, "big") + bytes(me), 0)


def callsign_mb(text):
    """BDS 2,0: the register byte and eight characters of CHARSET's"""
    v = 0
    for ch in text:
        v = v << 6 | CHARSET.index(ch)
    return bytes([0x20]) + v.to_bytes(6, "big")
