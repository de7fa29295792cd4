"""The gate of the Mode S model itself (tests/modes_model.py), which the CPU mirror and the device are judged by: the
Gillham code's defining properties, the 25 ft code, the squawk, the CRC against the project's own and a known frame."""
import ctypes as C

import numpy as np

from tests import modes_model as M

KNOWN_FRAME = bytes.fromhex("8D4840D6202CC371C32CE0576098")


def _gillham_codes():
    """every 13-bit field with M = Q = 0: 2^11 of them"""
    return [f for f in range(1 << 13) if not f & M.field_of(M=1, Q=1)]


def test_gillham_is_a_unit_distance_bijection_onto_minus_1200_to_126700():
    codes = _gillham_codes()
    assert len(codes) == 2048
    feet = {f: M.gillham(f) for f in codes}
    valid = {f: a for f, a in feet.items() if a is not None}
    assert len(valid) == 1280
    assert sorted(valid.values()) == list(range(-1200, 126701, 100))              # one-to-one and onto
    by_altitude = {a: f for f, a in valid.items()}
    for a in range(-1200, 126700, 100):
        assert bin(by_altitude[a] ^ by_altitude[a + 100]).count("1") == 1, a      # neighbours differ in one bit
    assert M.gillham(M.field_of(C4=1)) == -1200 and by_altitude[-1200] == M.field_of(C4=1)
    # and through the AC field's front door, where f == 0 stands for no altitude at all
    assert M.altitude(0) == (0, 0) and M.altitude(M.field_of(C4=1)) == (M.ALT, -1200)
    assert sum(M.altitude(f)[0] == M.ALT for f in codes) == 1280


def test_25_foot_code_and_the_metric_bit():
    with_q = [f for f in range(1 << 13) if f & M.field_of(Q=1) and not f & M.field_of(M=1)]
    got = sorted(M.altitude(f)[1] for f in with_q)
    assert all(M.altitude(f)[0] == M.ALT for f in with_q)
    assert got == list(range(-1000, 50176, 25)) and len(with_q) == 2048
    assert all(M.altitude(f) == (M.ALT_METRIC, 0) for f in range(1 << 13) if f & M.field_of(M=1))
    # the formula of the definition, digit for digit
    for f in with_q[::37]:
        n = (f & 0x1F80) >> 2 | (f & 0x20) >> 1 | (f & 0xF)
        assert M.altitude(f)[1] == 25 * n - 1000


def test_every_id_code_is_an_octal_squawk():
    ids = [f for f in range(1 << 13) if not f & 0x40]
    got = [M.squawk(f) for f in ids]
    octal = sorted(1000 * a + 100 * b + 10 * c + d for a in range(8) for b in range(8) for c in range(8) for d in range(8))
    assert len(ids) == 4096 and sorted(got) == octal
    assert {7700, 7600, 7500} <= set(got)
    assert M.squawk(M.field_of(A4=1, A2=1, A1=1, B4=1, B2=1, B1=1)) == 7700
    assert M.squawk(M.field_of(C1=1)) == 10 and M.squawk(M.field_of(D1=1)) == 1 and M.squawk(M.field_of(B4=1)) == 400
    assert all(M.squawk(f | 0x40) == M.squawk(f) for f in ids[::53])              # the zero bit is not read


def test_crc_agrees_with_the_projects_and_with_itself(lib):
    from air_rs_amd import _lib
    rng = np.random.default_rng(11)
    rows = rng.integers(0, 256, size=(500, 11)).astype(np.uint8)
    many = M.crc24_many(rows)
    assert [M.crc24(r.tobytes()) for r in rows] == many.tolist()
    assert M.crc24_many(rows[:, :4]).tolist() == [M.crc24(r[:4].tobytes()) for r in rows]
    # the project's crc24_11, through the wire input's CRC filter: a frame passes exactly with the model's parity
    fn = _lib.load().adsb_host_wire_parse
    cfg = _lib.AdsbWireInCfg(_lib.ADSB_WIRE_BEAST, _lib.ADSB_WIRE_IN_CRC, 0, 0, 0, 0)
    for r, crc in zip(rows[:200], many[:200]):
        for parity, kept in ((int(crc), 1), (int(crc) ^ 1, 0)):
            body = (bytes(7) + r.tobytes() + parity.to_bytes(3, "big")).replace(b"\x1a", b"\x1a\x1a")
            stream, end, n = b"\x1a3" + body, C.c_uint64(), C.c_size_t()
            end.value = len(stream)
            assert fn(C.byref(cfg), stream, len(stream), C.byref(end), 1, None, None, None, 4, C.byref(n), None, None, None) == 0
            assert n.value == kept


def test_the_known_frame_is_self_with_its_address(lib):
    assert M.syndrome(KNOWN_FRAME) == 0
    got = M.modes([KNOWN_FRAME])
    M.same(lib.host_modes(M.frame_list([KNOWN_FRAME])), got, "the CPU mirror")
    assert got["recs"]["kind"].tolist() == [M.SELF] and got["recs"]["address"].tolist() == [0x4840D6]
    assert got["known_out"].tolist() == [0x4840D6] and len(got["squitters"]) == 1 and got["recs"]["ca"].tolist() == [5]
    assert M.overlay(KNOWN_FRAME[:11], 0) == KNOWN_FRAME


def test_the_known_rule_is_causal():
    a = 0x123456
    got = M.modes([M.reply(4, a), M.all_call(a), M.reply(4, a)])
    assert got["recs"]["kind"].tolist() == [M.UNKNOWN, M.SELF, M.KNOWN] and got["recs"]["address"].tolist() == [a] * 3
    assert M.modes([M.reply(4, a)], [a])["recs"]["kind"].tolist() == [M.KNOWN]
