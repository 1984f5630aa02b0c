// Lane-interleaved rANS coder core of the "lanes" stream format (csrc/rans_lanes.hip,
// DESIGN.md section 25).
//
// A group of at most W * K symbols is coded by W independent rANS lanes; symbol j belongs to
// lane j % W at step j / W.  A lane is a 32-bit state with byte renormalisation,
// x in [2^23, 2^31), over the 16-bit CDF tables, escape symbol and 4-bit bypass digits of
// csrc/rans_chunk.h; the record sequence per symbol is that of chunk_encode / chunk_decode
// (CDF record, digit count, digits low to high).  All lanes share ONE byte stream, ordered by
// the decoder's reads: (step, record, round, lane).  After record r every lane that needs a
// byte takes one in ascending lane order (round 1), then every lane that still needs one
// (round 2); a lane's place in a round is the count of set bits below it in the round's lane
// mask.  The encoder walks steps and records backwards and fills the stream from its end:
// round-2 bytes, then round-1 bytes, each in descending lane order.  A group's bytes are the W
// final states (little-endian u32, lane order; L for a lane without symbols), then the stream.
//
// This file holds what a lane computes (shared, unchanged, by the CPU loops below and by the
// GPU lanes of rans_lanes.hip) and the group coder written as loops over the W lanes, where
// the "lane mask -> prefix count" primitive is a loop too; on the device it is a wave ballot.
// As in rans_chunk.h: no HIP header, no trap, every read bounded by the arguments (a byte past
// the group's end reads as 0 and records a code), no loop on stream content without a bound.
#ifndef RGBAC_RANS_LANES_H_
#define RGBAC_RANS_LANES_H_
#include <stdint.h>

#include "rans_chunk.h"

namespace rgbac_lanes {

namespace rr = rgbac_rans;

constexpr uint32_t kL = 1u << 23;               // lower bound of a lane's state
constexpr uint32_t kTop = 1u << 31;             // states stay below it
constexpr int kMaxLanes = 64;
constexpr int kMaxRecords = rr::kMaxRecords;    // CDF record, digit count, 8 digits

RGBAC_HD inline bool lanes_ok(int W) { return W == 8 || W == 16 || W == 32 || W == 64; }

// bytes a group of n symbols can take at most: the states, two bytes per CDF record, one per
// digit record
RGBAC_HD inline int64_t group_bound(int64_t n, int W) { return 4 * (int64_t)W + 11 * n; }

// CDF rows as the coder reads them: entry k of row ci modulo 2^16.  The rows hold exclusive
// sums, so only the closing 2^16 of a row wraps (to 0), and neither coder reads it as a bound:
// the search runs over the size - 1 sums and a frequency is a difference modulo 2^16.
struct RowsI32 {                                // the int32 [ncdf][stride] table of rans.cpp
  const int32_t* cdfs;
  int32_t stride;
  RGBAC_HD uint32_t at(int32_t ci, int32_t k) const {
    return (uint32_t)cdfs[(int64_t)ci * stride + k] & 0xFFFFu;
  }
};
struct RowsU16 {                                // the same entries staged as u16 (LDS)
  const uint16_t* cdfs;
  int32_t stride;
  RGBAC_HD uint32_t at(int32_t ci, int32_t k) const { return cdfs[ci * stride + k]; }
};

// the records of one symbol: nrec = 0 (nothing to code), 1 (CDF record) or 2 + digits
struct Rec {
  uint32_t start, freq, raw;
  int32_t nrec;
};

template <class Rows>
RGBAC_HD inline Rec make_record(int32_t sym, int32_t ci, int32_t size, int32_t offset,
                                const Rows& rows, int32_t* err) {
  const int32_t max_value = size - 2;
  int64_t value = (int64_t)sym - offset;
  uint32_t raw = 0;
  if (value < 0) {
    raw = (uint32_t)(-2 * value - 1);
    value = max_value;
  } else if (value >= max_value) {
    raw = (uint32_t)(2 * (value - max_value));
    value = max_value;
  }
  Rec r = {0, 0, raw, 1};
  if (value == max_value) {
    int32_t nb = 0;
    while (nb < rr::kMaxBypass && (raw >> (nb * rr::kBypassBits)) != 0) ++nb;
    r.nrec = 2 + nb;
  }
  r.start = rows.at(ci, (int32_t)value);
  r.freq = (rows.at(ci, (int32_t)value + 1) - r.start) & 0xFFFFu;
  if (r.freq == 0) {                            // not a CDF: nothing sane to emit, no division
    if (!*err) *err = rr::kErrCorrupt;
    r.nrec = 0;
  }
  return r;
}

// encoder: the bytes record r sheds first (0..2 for the CDF record, 0..1 for a digit)
RGBAC_HD inline int32_t enc_shifts(uint32_t x, int32_t r, uint32_t freq) {
  const uint32_t x_max = r == 0 ? freq << 15 : 1u << 27;
  return (int32_t)(x >= x_max) + (int32_t)((x >> 8) >= x_max);
}

// encoder: record r of rec pushed onto the renormalised state
RGBAC_HD inline uint32_t enc_apply(uint32_t x, int32_t r, const Rec& rec) {
  if (r == 0) {
    const uint32_t q = x / rec.freq;
    return (q << rr::kPrecision) + (x - q * rec.freq) + rec.start;
  }
  const uint32_t v = r == 1 ? (uint32_t)(rec.nrec - 2)
                            : (rec.raw >> ((r - 2) * rr::kBypassBits)) & rr::kMaxBypassVal;
  return (x << rr::kBypassBits) | v;
}

// decoder: pops the CDF record of row ci -> the state before renormalisation; *s = the symbol
template <class Rows>
RGBAC_HD inline uint32_t dec_cdf(uint32_t x, int32_t ci, int32_t size, const Rows& rows,
                                 int32_t* s, int32_t* err) {
  const uint32_t cum = x & 0xFFFFu;
  int32_t first = 0, len = size - 1;            // upper_bound over the exclusive sums
  while (len > 0) {
    const int32_t half = len >> 1;
    if (rows.at(ci, first + half) <= cum) {
      first += half + 1;
      len -= half + 1;
    } else {
      len = half;
    }
  }
  *s = first > 0 ? first - 1 : 0;
  const uint32_t start = rows.at(ci, *s);
  const uint32_t freq = (rows.at(ci, *s + 1) - start) & 0xFFFFu;
  if (first == 0 || freq == 0) {
    if (!*err) *err = rr::kErrCorrupt;
    return x;
  }
  return freq * (x >> rr::kPrecision) + cum - start;
}

// decoder: bytes to shift in after a record (a state below 2^7 cannot come back: corrupt)
RGBAC_HD inline int32_t dec_need(uint32_t x) {
  return (int32_t)(x < kL) + (int32_t)(x < (1u << 15));
}

RGBAC_HD inline int32_t escape_value(uint32_t raw, int32_t max_value) {
  const uint32_t mag = raw >> 1;
  return (int32_t)((raw & 1) ? ~mag : mag + (uint32_t)max_value);   // -mag - 1 == ~mag
}

// the row of symbol index ci, clamped into the tables; false (and a code) if it was not valid
RGBAC_HD inline bool row_of(const rr::Tables& t, int32_t* ci, int32_t* size, int32_t* offset,
                            int32_t* err) {
  bool ok = true;
  if (*ci < 0 || *ci >= t.ncdf) {
    if (!*err) *err = rr::kErrIndex;
    *ci = rr::detail::clamp_i32(*ci, 0, t.ncdf - 1);
    ok = false;
  }
  *size = t.sizes[*ci];
  if (*size < 3 || *size > t.stride) {
    if (!*err) *err = rr::kErrCorrupt;
    *size = rr::detail::clamp_i32(*size, 3, t.stride);
    ok = false;
  }
  *offset = t.offsets[*ci];
  return ok;
}

// ------------------------------------------------------------------ the group coder, on a CPU
// lane mask -> count of set lanes below / above lane l: the loop the device replaces by a ballot
inline int32_t count_below(const bool* mask, int32_t l) {
  int32_t c = 0;
  for (int32_t i = 0; i < l; ++i) c += mask[i];
  return c;
}
inline int32_t count_above(const bool* mask, int32_t l, int32_t W) {
  int32_t c = 0;
  for (int32_t i = l + 1; i < W; ++i) c += mask[i];
  return c;
}

// Encodes sym[0..n) / idx[0..n) as one group of W lanes, filling bytes backwards from ``end``
// (nullptr: count only).  Returns the group's byte count, states included; at most ``cap``
// bytes are stored, all inside [end - cap, end).  A bad index or row is clamped / skipped and
// recorded in *err (first code wins).
inline int64_t group_encode(const int32_t* sym, const int32_t* idx, int64_t n, int32_t W,
                            const rr::Tables& t, uint8_t* end, int64_t cap, int32_t* err) {
  const RowsI32 rows = {t.cdfs, t.stride};
  uint32_t x[kMaxLanes];
  Rec rec[kMaxLanes];
  int32_t c[kMaxLanes];
  bool m1[kMaxLanes], m2[kMaxLanes];
  for (int32_t l = 0; l < W; ++l) x[l] = kL;
  int64_t nb = 0;                               // bytes written so far, counted from end
  auto store = [&](int64_t back, uint32_t b) {  // the byte ``back`` places below end
    if (end && back <= cap) end[-back] = (uint8_t)b;
  };
  const int64_t steps = (n + W - 1) / W;
  for (int64_t step = steps - 1; step >= 0; --step) {
    int32_t maxrec = 0;
    for (int32_t l = 0; l < W; ++l) {
      const int64_t j = step * W + l;
      rec[l].nrec = 0;
      if (j >= n) continue;
      int32_t ci = idx[j], size, offset;
      row_of(t, &ci, &size, &offset, err);
      rec[l] = make_record(sym[j], ci, size, offset, rows, err);
      if (rec[l].nrec > maxrec) maxrec = rec[l].nrec;
    }
    for (int32_t r = maxrec - 1; r >= 0; --r) {
      for (int32_t l = 0; l < W; ++l) {
        c[l] = rec[l].nrec > r ? enc_shifts(x[l], r, rec[l].freq) : 0;
        m1[l] = c[l] >= 1;
        m2[l] = c[l] == 2;
      }
      const int32_t n2 = count_below(m2, W), n1 = count_below(m1, W);
      for (int32_t l = 0; l < W; ++l) {
        if (m2[l]) store(nb + 1 + count_above(m2, l, W), x[l] & 255);
        if (m1[l]) store(nb + n2 + 1 + count_above(m1, l, W), (m2[l] ? x[l] >> 8 : x[l]) & 255);
      }
      nb += n2 + n1;
      for (int32_t l = 0; l < W; ++l)
        if (rec[l].nrec > r) x[l] = enc_apply(x[l] >> (8 * c[l]), r, rec[l]);
    }
  }
  for (int32_t l = 0; l < W; ++l)
    for (int32_t b = 0; b < 4; ++b) store(nb + 4 * (W - l) - b, (x[l] >> (8 * b)) & 255);
  return nb + 4 * W;
}

// Decodes the n symbols of idx[0..n) from the group bytes[0..nbytes) into out[0..n).  Returns
// 0 or the first error code; from the step of an error on, out is 0.  At the end every lane
// must be back at L with every byte consumed (kErrCorrupt otherwise).
inline int32_t group_decode(const uint8_t* bytes, int64_t nbytes, const int32_t* idx, int64_t n,
                            int32_t W, const rr::Tables& t, int32_t* out) {
  const RowsI32 rows = {t.cdfs, t.stride};
  uint32_t x[kMaxLanes], raw[kMaxLanes];
  int32_t need[kMaxLanes], s[kMaxLanes], size[kMaxLanes], offset[kMaxLanes], nd[kMaxLanes];
  bool mask[kMaxLanes], esc[kMaxLanes];
  int32_t err = rr::kErrNone;
  if (nbytes < 0) nbytes = 0;
  int64_t pos = 0;
  auto byte_at = [&](int64_t p) -> uint32_t {
    if (p >= nbytes) {
      if (!err) err = rr::kErrPastEnd;
      return 0;
    }
    return bytes[p];
  };
  // two rounds of reads after a record: need[l] bytes for lane l
  auto rounds = [&]() {
    for (int32_t round = 1; round <= 2; ++round) {
      for (int32_t l = 0; l < W; ++l) mask[l] = need[l] >= round;
      for (int32_t l = 0; l < W; ++l)
        if (mask[l]) x[l] = (x[l] << 8) | byte_at(pos + count_below(mask, l));
      pos += count_below(mask, W);
    }
    for (int32_t l = 0; l < W; ++l)
      if (need[l] && x[l] < kL && !err) err = rr::kErrCorrupt;
  };
  for (int32_t l = 0; l < W; ++l) {
    x[l] = 0;
    for (int32_t b = 0; b < 4; ++b) x[l] |= byte_at(4 * l + b) << (8 * b);
    if ((x[l] < kL || x[l] >= kTop) && !err) err = rr::kErrCorrupt;
  }
  pos = 4 * (int64_t)W;
  const int64_t steps = (n + W - 1) / W;
  int64_t step = 0;
  for (; step < steps && !err; ++step) {
    bool any_esc = false;
    for (int32_t l = 0; l < W; ++l) {
      const int64_t j = step * W + l;
      need[l] = 0;
      esc[l] = false;
      raw[l] = 0;
      nd[l] = 0;
      if (j >= n) continue;
      int32_t ci = idx[j];
      if (!row_of(t, &ci, &size[l], &offset[l], &err)) continue;
      int32_t e = rr::kErrNone;
      x[l] = dec_cdf(x[l], ci, size[l], rows, &s[l], &e);
      if (e) {
        if (!err) err = e;
        continue;
      }
      need[l] = dec_need(x[l]);
      esc[l] = s[l] == size[l] - 2;
      any_esc |= esc[l];
    }
    rounds();
    if (any_esc && !err) {
      for (int32_t l = 0; l < W; ++l) {                     // the digit count
        need[l] = 0;
        if (!esc[l]) continue;
        nd[l] = (int32_t)(x[l] & rr::kMaxBypassVal);
        x[l] >>= rr::kBypassBits;
        need[l] = x[l] < kL;
        if (nd[l] > rr::kMaxBypass) {
          if (!err) err = rr::kErrBypass;
          nd[l] = 0;
        }
      }
      rounds();
      for (int32_t j = 0; j < rr::kMaxBypass && !err; ++j) {
        bool any = false;
        for (int32_t l = 0; l < W; ++l) {
          need[l] = 0;
          if (!esc[l] || j >= nd[l]) continue;
          any = true;
          raw[l] |= (x[l] & rr::kMaxBypassVal) << (j * rr::kBypassBits);
          x[l] >>= rr::kBypassBits;
          need[l] = x[l] < kL;
        }
        if (!any) break;
        rounds();
      }
    }
    if (err) break;
    for (int32_t l = 0; l < W; ++l) {
      const int64_t j = step * W + l;
      if (j >= n) continue;
      const int32_t v = esc[l] ? escape_value(raw[l], size[l] - 2) : s[l];
      out[j] = (int32_t)((uint32_t)v + (uint32_t)offset[l]);
    }
  }
  if (err) {
    for (int64_t j = step * W; j < n; ++j) out[j] = 0;
    return err;
  }
  for (int32_t l = 0; l < W; ++l)
    if (x[l] != kL) err = rr::kErrCorrupt;
  if (pos != nbytes) err = rr::kErrCorrupt;
  return err;
}

}  // namespace rgbac_lanes
#endif  // RGBAC_RANS_LANES_H_
