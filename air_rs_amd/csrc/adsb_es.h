// adsb_es.h -- what the ME field of one DF17/18 frame says about the aircraft beside identity, position and velocity
// (include/adsb_hip.h, "Extended squitter status"): the state its format, type code and subtype give it, the fields of
// that state, and the integrity table (include/adsb_host.h, adsb_host_es_integrity).  One text for the device
// (adsb_es.hip) and the CPU mirror (host/adsb_es.cpp, adsb_host_es): every function here is __host__ __device__ under
// hipcc and plain inline C++ otherwise.  Integers only.  Built on adsb_modes.h's ModesBytes: ME is one 56-bit number cut
// from the frame's two words, every field a shift and a mask of it, so a frame stays in registers and no array is
// indexed by a variable.
#ifndef ADSB_ES_H
#define ADSB_ES_H

#include <stdint.h>

#include "../../include/adsb_hip.h"
#include "adsb_modes.h"

namespace adsbk {

constexpr uint32_t kEsVersions = 4; // the header's version totals: 0, 1, 2 and 3-7
// the header's totals as the kernels count them: the states, then the OPERATIONAL records of each version
constexpr uint32_t kEsTallies = ADSB_ES_STATES + kEsVersions;

// ME, bit 1 in bit 55 of v
struct EsMe {
    uint64_t v;
    // u(a, n), n <= 32
    ADSB_WIRE_HD uint32_t u(uint32_t a, uint32_t n) const { return (uint32_t)((v >> (57u - a - n)) & ((1ull << n) - 1ull)); }
};
ADSB_WIRE_HD inline EsMe es_me(const ModesBytes &b) { return EsMe{(b.w0 & 0xFFFFFFFFull) << 24 | b.w1 >> 40}; }

struct EsIntegrity {
    uint32_t nic, rc_dm; // rc_dm 0: unknown
};

// NIC and Rc in decimetres of a position message with type code tc from an aircraft of this version; supp: bit 0 = A,
// bit 1 = B, bit 2 = C.  The table of include/adsb_host.h, row by row
ADSB_WIRE_HD inline EsIntegrity es_integrity(uint32_t tc, uint32_t version, uint32_t supp)
{
    const uint32_t v = version == ADSB_ES_VERSION_UNKNOWN ? 0u : version >= 2u ? 2u : version;
    const bool a = supp & 1u, b = (supp & 2u) && v == 2u, c = (supp & 4u) && v == 2u;
    const bool ab = v == 2u ? a && b : a; // "A (v1) or A and B (v2)"
    EsIntegrity r{0u, 0u};
    switch (tc) {
    case 9: case 20: case 5: r = EsIntegrity{11u, 75u}; break;
    case 10: case 21: case 6: r = EsIntegrity{10u, 250u}; break;
    case 11: r = v && ab ? EsIntegrity{9u, 750u} : EsIntegrity{8u, 1852u}; break;
    case 12: r = EsIntegrity{7u, 3704u}; break;
    case 13: r = EsIntegrity{6u, v && a ? 11112u : b ? 5556u : 9260u}; break;
    case 14: r = EsIntegrity{5u, 18520u}; break;
    case 15: r = EsIntegrity{4u, 37040u}; break;
    case 16: r = v == 0u ? EsIntegrity{0u, 185200u} : ab ? EsIntegrity{3u, 74080u} : EsIntegrity{2u, 148160u}; break;
    case 17: r = EsIntegrity{1u, 370400u}; break;
    case 7: r = v && a && !c ? EsIntegrity{9u, 750u} : EsIntegrity{8u, 1852u}; break;
    case 8:
        if (v == 2u) r = a && c ? EsIntegrity{7u, 3704u} : a ? EsIntegrity{6u, 5556u} : c ? EsIntegrity{6u, 11112u} : EsIntegrity{0u, 0u};
        break;
    default: break;
    }
    if (v == 0u) r.nic = 0u;
    return r;
}

// field x of r holds `expr`
#define ADSB_ES_SET(field, has, expr)         \
    do {                                      \
        r.field = (expr);                     \
        present |= (has);                     \
    } while (0)

// The record of one frame.  Every byte of it is written.
ADSB_WIRE_HD inline adsb_es_rec es_first(const ModesBytes &b)
{
    adsb_es_rec r{};
    const uint32_t df = b[0] >> 3;
    if (df != 17u && df != 18u) return r; // ADSB_ES_NOT_ES = 0
    if (df == 18u && (b[0] & 7u) > 1u) {
        r.state = ADSB_ES_FOREIGN;
        return r;
    }
    const EsMe m = es_me(b);
    const uint32_t tc = m.u(1, 5), st = m.u(6, 3);
    uint32_t state = ADSB_ES_RESERVED, subtype = tc == 29u ? st >> 1 : st, present = 0, flags = 0;
    if (tc >= 1u && tc <= 4u) {
        state = ADSB_ES_CATEGORY;
        subtype = 0;
        ADSB_ES_SET(category, ADSB_ES_HAS_CATEGORY, (uint8_t)((0xEu - tc) << 4 | st));
    } else if (tc <= 18u || (tc >= 20u && tc <= 22u)) {
        state = ADSB_ES_POSITION;
        subtype = 0;
        if (tc >= 9u && tc <= 18u) ADSB_ES_SET(nic_b, ADSB_ES_HAS_NIC_B, (uint8_t)m.u(8, 1));
        const uint32_t rc = es_integrity(tc, 0u, 0u).rc_dm;
        if (rc) ADSB_ES_SET(value, ADSB_ES_HAS_RC, rc);
    } else if (tc == 19u && st >= 1u && st <= 4u) {
        state = ADSB_ES_VELOCITY;
        ADSB_ES_SET(nac_v, ADSB_ES_HAS_NAC_V, (uint8_t)m.u(11, 3));
        flags = (m.u(9, 1) ? ADSB_ES_INTENT_CHANGE : 0u) | (m.u(10, 1) ? ADSB_ES_IFR : 0u);
        present |= ADSB_ES_HAS_VELOCITY_FLAGS;
    } else if (tc == 28u && st == 1u) {
        state = ADSB_ES_EMERGENCY;
        ADSB_ES_SET(emergency, ADSB_ES_HAS_EMERGENCY, (uint8_t)m.u(9, 3));
        ADSB_ES_SET(half[0], ADSB_ES_HAS_SQUAWK, (uint16_t)modes_squawk(m.u(12, 13)));
    } else if (tc == 28u && st == 2u) {
        state = ADSB_ES_ACAS_RA;
        r.value = m.u(9, 32);
        r.half[0] = (uint16_t)m.u(41, 16);
        present = ADSB_ES_HAS_RA;
    } else if (tc == 29u && subtype == 1u) {
        state = ADSB_ES_TARGET_STATE;
        ADSB_ES_SET(version, ADSB_ES_HAS_VERSION, 2);
        ADSB_ES_SET(sil_supplement, ADSB_ES_HAS_SIL_SUPPLEMENT, (uint8_t)m.u(8, 1));
        const uint32_t alt = m.u(10, 11), baro = m.u(21, 9);
        if (alt) ADSB_ES_SET(value, ADSB_ES_HAS_SELECTED_ALT, 32u * (alt - 1u));
        if (baro) ADSB_ES_SET(half[0], ADSB_ES_HAS_BARO, (uint16_t)(8000u + 8u * (baro - 1u)));
        if (m.u(30, 1)) ADSB_ES_SET(half[1], ADSB_ES_HAS_HEADING, (uint16_t)m.u(31, 9));
        ADSB_ES_SET(nac_p, ADSB_ES_HAS_NAC_P, (uint8_t)m.u(40, 4));
        ADSB_ES_SET(nic_baro, ADSB_ES_HAS_NIC_BARO, (uint8_t)m.u(44, 1));
        ADSB_ES_SET(sil, ADSB_ES_HAS_SIL, (uint8_t)m.u(45, 2));
        flags = (m.u(9, 1) ? ADSB_ES_ALT_FMS : 0u) | (m.u(53, 1) ? ADSB_ES_TCAS : 0u);
        present |= ADSB_ES_HAS_ALT_SOURCE | ADSB_ES_HAS_TCAS;
        if (m.u(47, 1)) {
            flags |= (m.u(48, 1) ? ADSB_ES_AUTOPILOT : 0u) | (m.u(49, 1) ? ADSB_ES_VNAV : 0u) | (m.u(50, 1) ? ADSB_ES_ALT_HOLD : 0u) |
                     (m.u(52, 1) ? ADSB_ES_APPROACH : 0u) | (m.u(54, 1) ? ADSB_ES_LNAV : 0u);
            present |= ADSB_ES_HAS_MODES;
        }
    } else if (tc == 31u && st <= 1u) {
        state = ADSB_ES_OPERATIONAL;
        const uint32_t version = m.u(41, 3);
        ADSB_ES_SET(version, ADSB_ES_HAS_VERSION, (uint8_t)version);
        if (version <= 2u) {
            r.half[0] = (uint16_t)m.u(9, 16);
            r.half[1] = (uint16_t)m.u(25, 16);
            present |= ADSB_ES_HAS_CC_OM;
        }
        if (version == 1u || version == 2u) {
            ADSB_ES_SET(nic_a, ADSB_ES_HAS_NIC_A, (uint8_t)m.u(44, 1));
            ADSB_ES_SET(nac_p, ADSB_ES_HAS_NAC_P, (uint8_t)m.u(45, 4));
            ADSB_ES_SET(sil, ADSB_ES_HAS_SIL, (uint8_t)m.u(51, 2));
            flags = m.u(54, 1) ? ADSB_ES_HRD : 0u;
            present |= ADSB_ES_HAS_HRD;
            if (st == 0u) {
                ADSB_ES_SET(nic_baro, ADSB_ES_HAS_NIC_BARO, (uint8_t)m.u(53, 1));
            } else {
                flags |= m.u(53, 1) ? ADSB_ES_TRACK_HEADING : 0u;
                present |= ADSB_ES_HAS_TRACK_HEADING;
                ADSB_ES_SET(length_width, ADSB_ES_HAS_LENGTH_WIDTH, (uint8_t)m.u(21, 4));
            }
        }
        if (version == 2u) {
            ADSB_ES_SET(sil_supplement, ADSB_ES_HAS_SIL_SUPPLEMENT, (uint8_t)m.u(55, 1));
            ADSB_ES_SET(sda, ADSB_ES_HAS_SDA, (uint8_t)m.u(31, 2));
            if (st == 0u) {
                ADSB_ES_SET(gva, ADSB_ES_HAS_GVA, (uint8_t)m.u(49, 2));
            } else {
                ADSB_ES_SET(nic_c, ADSB_ES_HAS_NIC_C, (uint8_t)m.u(20, 1));
                ADSB_ES_SET(nac_v, ADSB_ES_HAS_NAC_V, (uint8_t)m.u(17, 3));
            }
        }
    }
    r.state = (uint8_t)state;
    r.type_code = (uint8_t)tc;
    r.subtype = (uint8_t)subtype;
    r.present = present;
    r.flags = (uint16_t)flags;
    return r;
}
#undef ADSB_ES_SET

// which of the kEsTallies totals a record counts for beside its state's: the version's place for OPERATIONAL, else none
ADSB_WIRE_HD inline uint32_t es_version_tally(const adsb_es_rec &r)
{
    if (r.state != ADSB_ES_OPERATIONAL) return 0xFFu;
    return ADSB_ES_STATES + (r.version < 3u ? r.version : 3u);
}

// the header from the kEsTallies totals of an n-frame list
ADSB_WIRE_HD inline void es_header_of(uint64_t n, const uint64_t *t, adsb_es_header *h)
{
    h->n = n;
    for (uint32_t k = 0; k < ADSB_ES_STATES; ++k) h->n_state[k] = t[k];
    for (uint32_t k = 0; k < kEsVersions; ++k) h->n_version[k] = t[ADSB_ES_STATES + k];
    h->reserved = 0;
}

// The argument rule both entry points share (host code)
inline int es_args_check(const adsb_frame *frames, size_t n)
{
    if (!frames && n) return ADSB_E_ARG;
    if ((uint64_t)n > 0xFFFFFFFFull) return ADSB_E_CAPACITY;
    return ADSB_OK;
}

} // namespace adsbk

#endif
