"""The lists a track table's extended squitter side is checked on (tests/test_track_es_host.py on the CPU mirror,
tests/test_gpu_track_es.py on the device), built with tests/es_cases.py's / tests/es_model.py's frame makers.  A case is
dict(name, frames, es, recs, claim): a FRAME_DTYPE list, its stateless adsb_es_rec records and, for the keyed path, its
adsb_modes_rec records (the models', so no library call is needed to build a case), and the claim the list is there to
show: [(frame index, {field of the per-frame output: value, "has": flags, "lacks": flags})].  claims_hold() asserts every
claim against the MODEL's result, so a list cannot quietly stop showing it."""
import numpy as np

from tests import es_cases as E
from tests import es_model as M
from tests import modes_model as MM
from tests import track_es_model as T

SPS = 0.5e-6
STEP = 2000                                  # samples between frames: 1 ms
A, B = 0x4840D6, 0x3C6586
FLAG = dict(COUNTED=T.COUNTED, POSITION=T.POSITION, VERSIONED=T.VERSIONED, STALE_A=T.STALE_A, STALE_C=T.STALE_C)
SECOND = 2_000_000                           # samples


# ---- frames ------------------------------------------------------------------------------------------------------------
def position(icao, tc, nic_b=0, df=17, low3=5):
    """a position message of type code tc; bit 8 of ME (NIC supplement B on TC 9-18) as given"""
    return M.frame(M.me_tc(tc, st=nic_b, rest=0x2CC371C32CE0), df=df, low3=low3, aa=icao)


def status(icao, version=2, nic_a=0, surface=False, nic_c=0, nac_v=0, nac_p=9, sil=3):
    """an operational status message (TC 31; ST 1 with surface), NIC supplement C and NACv in the surface capability codes"""
    cc = (nic_c << 4 | nac_v << 5) if surface else 0
    return M.frame(M.me_operational(st=int(surface), version=version, cc=cc, nic_a=nic_a, nac_p=nac_p, sil=sil), aa=icao)


def target(icao, alt=532):
    return M.frame(M.me_target(alt=alt, baro=267, heading=95, nac_p=10, nic_baro=1, sil=2), aa=icao)


def emergency(icao, state=1, code=7700):
    return M.frame(M.me_emergency(state=state, code=code), aa=icao)


def acas_ra(icao, bits=0x812345678ABC):
    return M.frame(M.me_tc(28, 2, rest=bits), aa=icao)


def category(icao, tc=4, ca=3):
    return M.frame(M.me_tc(tc, st=ca, rest=0x0C3071C32CE0), aa=icao)


def velocity(icao, nac_v=2, ifr=1, intent=0):
    return M.frame(M.me_of({1: (5, 19), 6: (3, 1), 9: (1, intent), 10: (1, ifr), 11: (3, nac_v), 14: (43, 0x2AAAAAAAAAA)}), aa=icao)


def build(name, msgs, claim=None, offsets=None, kinds=None, addresses=None):
    """msgs in list order -> the case.  The keyed path's records: every DF17/18 frame SELF with its own address, any other
    format KNOWN with bytes[1..3] (as if resolved from the parity), unless kinds[j] says otherwise"""
    frames = M.frame_list(msgs)
    frames["offset"] = np.arange(len(msgs)) * STEP if offsets is None else np.asarray(offsets)
    recs = np.zeros(len(msgs), dtype=MM.REC_DTYPE)
    for j, msg in enumerate(msgs):
        df = msg[0] >> 3
        recs["address"][j], recs["df"][j] = int.from_bytes(msg[1:4], "big"), df
        if addresses is not None and addresses[j] is not None:
            recs["address"][j] = addresses[j]
        recs["kind"][j] = (MM.SELF if df in (17, 18) else MM.KNOWN) if kinds is None or kinds[j] is None else kinds[j]
    return dict(name=name, frames=frames, es=M.es(frames)["recs"], recs=recs, claim=claim)


def run_model(case, cuts=(), keyed=False, bases=None, **table):
    """The model over the case, cut at the given list positions -> (frame_es, records, the Table)"""
    t = T.Table(**table)
    edges = [0] + list(cuts) + [len(case["frames"])]
    outs = [t.update(case["frames"][a:b], case["es"][a:b], case["recs"][a:b] if keyed else None,
                     sample_base=0 if bases is None else bases[k]) for k, (a, b) in enumerate(zip(edges, edges[1:]))]
    return np.concatenate(outs) if outs else np.zeros(0, dtype=T.FRAME_ES_DTYPE), t.records(), t


def claims_hold(case, out=None, keyed=False, **table):
    if out is None:
        out = run_model(case, keyed=keyed, **table)[0]
    for j, want in case["claim"] or []:
        for key, v in want.items():
            if key == "has":
                assert all(int(out["flags"][j]) & FLAG[k] for k in v), (case["name"], j, key, v, out[j])
            elif key == "lacks":
                assert not any(int(out["flags"][j]) & FLAG[k] for k in v), (case["name"], j, key, v, out[j])
            else:
                assert int(out[key][j]) == v, (case["name"], j, key, v, out[j])


# ---- the known answers -------------------------------------------------------------------------------------------------
def known_answers():
    """every line of the table of known answers, each on an aircraft of its own so that nothing carries over"""
    rows = (  # (what is heard before the position, the position, NIC, Rc in dm)
        ([], (11, 0), 0, 1852),
        ([dict(version=2, nic_a=1)], (11, 1), 9, 750),
        ([dict(version=2, nic_a=1)], (11, 0), 8, 1852),
        ([dict(version=2, nic_a=0)], (13, 1), 6, 5556),
        ([dict(version=1, nic_a=1)], (13, 0), 6, 11112),
        ([dict(version=1, nic_a=1)], (16, 0), 3, 74080),
        ([dict(version=2, nic_a=1, surface=True, nic_c=0)], (7, 0), 9, 750),
        ([dict(version=2, nic_a=1, surface=True, nic_c=1)], (7, 0), 8, 1852),
        ([dict(version=2, nic_a=1, surface=True, nic_c=1)], (8, 0), 7, 3704),
        ([dict(version=1, nic_a=1, surface=True)], (8, 0), 0, 0),
    )
    msgs, claim = [], []
    for k, (before, (tc, nic_b), nic, rc) in enumerate(rows):
        icao = 0x500000 + k
        msgs += [status(icao, **kw) for kw in before] + [position(icao, tc, nic_b)]
        flags = dict(has=["COUNTED", "POSITION"] + (["VERSIONED"] if before else []), lacks=[] if before else ["VERSIONED"])
        claim.append((len(msgs) - 1, dict(nic=nic, rc_dm=rc, **flags)))
    return build("known answers", msgs, claim)


def status_after_the_position():
    """the operational status arrives AFTER the position in the same list: the position must not use it; the next one does"""
    msgs = [position(A, 11, 1), status(A, 2, nic_a=1), position(A, 11, 1)]
    return build("status after the position", msgs,
                 [(0, dict(nic=0, rc_dm=1852, version=M.VERSION_UNKNOWN, supp=2, lacks=["VERSIONED"])),
                  (1, dict(nic=0, rc_dm=0, version=M.VERSION_UNKNOWN, flags=T.COUNTED)),
                  (2, dict(nic=9, rc_dm=750, version=2, supp=3, has=["VERSIONED"]))])


def version_from_target_state():
    """a version from TARGET_STATE alone: version 2, no supplement A, so TC 13 with B reads 555.6 m and TC 11 stays NIC 8"""
    msgs = [target(A), position(A, 13, 1), position(A, 11, 1)]
    return build("version from target state", msgs,
                 [(1, dict(nic=6, rc_dm=5556, version=2, supp=2, has=["VERSIONED"], lacks=["STALE_A"])),
                  (2, dict(nic=8, rc_dm=1852, version=2, supp=2))])


AGE_SAMPLES = 120_000_000                    # 60 s of samples
AGE = float(AGE_SAMPLES) * SPS               # the frame time of a frame at that offset, and its age against one at 0


def age_edges():
    """with max_age_s = AGE: a supplement exactly max_age_s old is usable, one sample older is STALE (and with max_age_s one
    ulp below AGE the first one is STALE too: the tests reserve with nextafter(AGE, 0) for that).  The status is heard
    at time 0, so a position's age is its own frame time."""
    msgs = [status(A, 2, nic_a=1), position(A, 11, 1), position(A, 11, 1)]
    return build("age edges", msgs, offsets=[0, AGE_SAMPLES, AGE_SAMPLES + 1],
                 claim=[(1, dict(nic=9, rc_dm=750, supp=3, lacks=["STALE_A"])),
                        (2, dict(nic=8, rc_dm=1852, supp=2, has=["STALE_A", "VERSIONED"], version=2))])


def negative_age():
    """two updates, the later one with a smaller sample_base: the held supplements are from the 'future' and are STALE.
    -> (first, its sample_base, second, its sample_base)"""
    first = build("status at 10 s", [status(A, 2, nic_a=1, surface=True, nic_c=1)])
    second = build("position at 1 s", [position(A, 8)],
                   claim=[(0, dict(nic=0, rc_dm=0, supp=0, version=2, has=["STALE_A", "STALE_C", "VERSIONED"]))])
    return first, 10 * SECOND, second, SECOND


def infinite_age():
    msgs = [status(A, 2, nic_a=1), position(A, 11, 1)]
    return build("an hour later, max_age_s = +inf", msgs, offsets=[0, 3600 * SECOND],
                 claim=[(1, dict(nic=9, rc_dm=750, supp=3, lacks=["STALE_A"]))])


def version_zero_ignores_a():
    """a version-2 supplement A, then a version-0 status: A is still handed over (supp bit 0) and ignored by the table"""
    msgs = [status(A, 2, nic_a=1), position(A, 11, 1), status(A, 0), position(A, 11, 1)]
    return build("version 0 after version 2", msgs,
                 [(1, dict(nic=9, rc_dm=750, version=2, supp=3)),
                  (3, dict(nic=0, rc_dm=1852, version=0, supp=3, has=["VERSIONED"], lacks=["STALE_A"]))])


def interleaved():
    """two aircraft interleaved: each position reads its own aircraft's status"""
    msgs = [status(A, 2, nic_a=1), status(B, 1, nic_a=0), position(B, 11, 1), position(A, 11, 1), status(B, 1, nic_a=1),
            position(A, 16, 1), position(B, 16, 0), category(A), velocity(B)]
    return build("two aircraft interleaved", msgs,
                 [(2, dict(nic=8, rc_dm=1852, version=1, supp=2)), (3, dict(nic=9, rc_dm=750, version=2, supp=3)),
                  (5, dict(nic=3, rc_dm=74080, version=2)), (6, dict(nic=3, rc_dm=74080, version=1, supp=1))])


def foreign_is_not_counted():
    """DF18 with CF 2 is not counted (all zero); DF18 with CF 0 is"""
    msgs = [status(A, 2, nic_a=1), position(A, 11, 1, df=18, low3=2), position(A, 11, 1, df=18, low3=0)]
    return build("DF18 CF 2", msgs, [(1, dict(flags=0, rc_dm=0, nic=0, version=0, supp=0)), (2, dict(nic=9, rc_dm=750))])


def keyed_rejects():
    """the keyed path: a DF17 frame of kind PARITY is not counted, a DF20 reply of the aircraft is not counted"""
    reply = MM.reply(20, A, rest=bytes(7))
    msgs = [status(A, 2, nic_a=1), position(A, 11, 1), reply, position(A, 11, 1), position(B, 11, 1)]
    return build("keyed path rejects", msgs, kinds=[None, MM.PARITY, None, None, MM.UNKNOWN], addresses=[None, None, A, None, None],
                 claim=[(1, dict(flags=0, rc_dm=0)), (2, dict(flags=0)), (3, dict(nic=9, rc_dm=750)), (4, dict(flags=0))])


def every_block():
    """one aircraft says everything once: every block, the category and NACv get a home"""
    msgs = [category(A, 4, 3), status(A, 2, nic_a=1), status(A, 2, nic_a=0, surface=True, nic_c=1, nac_v=5), target(A),
            emergency(A, 1, 7700), acas_ra(A), velocity(A, nac_v=2, ifr=1), position(A, 8), position(A, 11, 1)]
    return build("every block", msgs, [(7, dict(nic=6, rc_dm=11112, supp=4)), (8, dict(nic=8, rc_dm=1852, supp=6))])


def twelve():
    """twelve frames of two aircraft, for every cut: statuses, positions that depend on them, and the other blocks"""
    msgs = [status(A, 2, nic_a=1), position(A, 11, 1), position(B, 13, 1), status(B, 1, nic_a=1), position(B, 13, 0),
            target(A), status(A, 2, nic_a=0, surface=True, nic_c=1), position(A, 8), velocity(B), emergency(A), position(B, 16),
            category(B)]
    return build("twelve frames", msgs,
                 [(1, dict(nic=9, rc_dm=750)), (2, dict(nic=0, rc_dm=9260)), (4, dict(nic=6, rc_dm=11112)),
                  (7, dict(nic=6, rc_dm=11112, supp=4)), (10, dict(nic=3, rc_dm=74080))])


def stateless_known():
    """the stateless stage's own known frames (tests/es_cases.py), five aircraft: each gets its blocks, none is versioned
    when its position is heard"""
    return build("the stateless stage's known frames", E.KNOWN_FRAMES,
                 [(4, dict(nic=0, rc_dm=1852, lacks=["VERSIONED"])), (5, dict(nic=0, rc_dm=1852, lacks=["VERSIONED"]))])


def small_cases():
    return [stateless_known(), known_answers(), status_after_the_position(), version_from_target_state(), version_zero_ignores_a(),
            interleaved(), foreign_is_not_counted(), every_block(), twelve()]


# ---- the seeded mix ----------------------------------------------------------------------------------------------------
POSITION_TCS = (0, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 20, 21, 22)


def mix(n, seed=11, n_aircraft=24, step=None):
    """n frames over n_aircraft aircraft: positions of every type code with either B, operational status of versions 0-3
    airborne and on the surface with every A and C, the other extended squitters, DF18 frames of other CF and short
    replies.  Every 97th gap is 61 s, so a held supplement goes stale now and then."""
    rng = np.random.default_rng(seed)
    msgs, offsets, t = [], [], 0
    for j in range(n):
        icao = 0x400000 + int(rng.integers(0, n_aircraft))
        kind = int(rng.integers(0, 16))
        if kind < 7:
            msgs.append(position(icao, int(rng.choice(POSITION_TCS)), int(rng.integers(0, 2))))
        elif kind < 11:
            msgs.append(status(icao, int(rng.choice((0, 1, 1, 2, 2, 2, 3))), int(rng.integers(0, 2)), bool(rng.integers(0, 2)),
                               int(rng.integers(0, 2)), int(rng.integers(0, 8))))
        elif kind == 11:
            msgs.append(target(icao, int(rng.integers(0, 2048))))
        elif kind == 12:
            msgs.append(emergency(icao, int(rng.integers(0, 8))) if rng.integers(0, 2) else acas_ra(icao, int(rng.integers(0, 1 << 48))))
        elif kind == 13:
            msgs.append(velocity(icao, int(rng.integers(0, 8)), int(rng.integers(0, 2)), int(rng.integers(0, 2))))
        elif kind == 14:
            msgs.append(category(icao, int(rng.integers(1, 5)), int(rng.integers(0, 8))))
        else:
            msgs.append(position(icao, 11, 1, df=18, low3=2) if rng.integers(0, 2) else MM.reply(20, icao, rest=bytes(7)))
        t += 61 * SECOND if j % 97 == 96 else (STEP if step is None else step)
        offsets.append(t)
    return build(f"mix of {n}", msgs, offsets=offsets)


V12_ROWS = {("row", k) for k, row in enumerate(T.ROWS) if row[1] in (1, 2)}


def reaches_everything(table):
    """through the table path the model has used every row of the integrity table for versions 1 and 2, and both STALE
    flags"""
    missing = (V12_ROWS | {"STALE_A", "STALE_C"}) - table.reached
    assert not missing, sorted((T.ROWS[m[1]] if isinstance(m, tuple) else m) for m in missing)


def one_aircraft_across_tiles(n=4097):
    """one aircraft, n frames: its status in the first scan tile, other frames between, positions in the last"""
    msgs = [status(A, 2, nic_a=1)] + [velocity(A, j & 7) for j in range(n - 4)] + [position(A, 11, 1), position(A, 13, 1), position(A, 16, 1)]
    step = 10_000                                                       # 5 ms: the last frame is 20.5 s after the first
    return build("one aircraft across tiles", msgs[:n], offsets=np.arange(n) * step,
                 claim=[(n - 3, dict(nic=9, rc_dm=750, lacks=["STALE_A"])), (n - 2, dict(nic=6, rc_dm=11112)),
                        (n - 1, dict(nic=3, rc_dm=74080))])


def many_aircraft(n=4097):
    """n aircraft of one frame each, alternating statuses and positions: nothing is resolved with anything"""
    msgs = [(position(0x100000 + 7 * j, 11, 1) if j & 1 else status(0x100000 + 7 * j, 2, nic_a=1)) for j in range(n)]
    return build("one frame each", msgs, claim=[(1, dict(nic=0, rc_dm=1852, lacks=["VERSIONED"]))])
