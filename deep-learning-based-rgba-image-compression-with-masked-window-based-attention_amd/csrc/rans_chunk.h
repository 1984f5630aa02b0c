// Per-chunk range-ANS coder core of the chunked stream format (csrc/rans_dev.hip, DESIGN.md
// "Device-side chunked rANS coder").
//
// One chunk is an independent rANS stream over at most K symbols, coded with the algorithm of
// csrc/rans.cpp (64-bit state, 32-bit renormalisation words, 16-bit CDFs, escape symbol +
// 4-bit bypass digits): the words of a chunk are exactly what rans.cpp's encoder flushes for
// the same symbols, so that coder is a byte-level oracle for every chunk.  The two state
// machines below are plain functions that run unchanged on the host and in a GPU lane:
//   * no HIP header, no global state, no trap (no assert, no division by an unchecked value);
//   * every read is bounded by the arguments: a stream word past the chunk's end reads as 0,
//     a CDF index outside [0, ncdf) is clamped, a table length outside [3, stride] is clamped,
//     and each of these records an error code;
//   * no loop runs on stream content without a bound.
// Compiles with a plain C++ compiler (tests/native/rans_chunk_check.cpp) and with hipcc.
#ifndef RGBAC_RANS_CHUNK_H_
#define RGBAC_RANS_CHUNK_H_
#include <stdint.h>

#if defined(__HIP__)
#define RGBAC_HD __attribute__((host)) __attribute__((device))
#else
#define RGBAC_HD
#endif

namespace rgbac_rans {

constexpr int kPrecision = 16;                  // CDF precision (bits)
constexpr int kBypassBits = 4;                  // bypass digit width
constexpr uint32_t kMaxBypassVal = 15;
constexpr int kMaxBypass = 8;                   // digits of a 32-bit raw value
constexpr uint64_t kL = 1ull << 31;             // lower bound of the state
constexpr int kMaxRecords = 2 + kMaxBypass;     // CDF record, digit count, digits

// error codes of the decoder (and of the encoder's index / table checks); 0 = none
enum : int32_t {
  kErrNone = 0,
  kErrPastEnd = 1,   // read past the end of the chunk's words
  kErrIndex = 2,     // CDF index outside [0, ncdf)
  kErrCorrupt = 3,   // corrupt stream or CDF table (search hit an end of the row, zero frequency)
  kErrBypass = 4,    // corrupt bypass length (> 8 digits)
  kErrChunk = 5,     // chunk table entry outside the caller's buffers
};

// cdfs[ncdf][stride] int32, row i valid up to sizes[i]; offsets[ncdf] (as in rans.cpp)
struct Tables {
  const int32_t* cdfs;
  int32_t stride;
  const int32_t* sizes;
  const int32_t* offsets;
  int32_t ncdf;
};

// words a chunk of n symbols can take at most: one per record plus the two state words
RGBAC_HD inline int64_t chunk_bound(int64_t n) { return (int64_t)kMaxRecords * n + 2; }

namespace detail {

struct EncState {
  uint64_t x;
  uint32_t* ptr;      // next word is stored at *--ptr; null in count-only mode
  int64_t cap;        // words the caller reserved below ``end``: no store beyond them
  int64_t nwords;
};

RGBAC_HD inline void emit(EncState& s, uint32_t w) {
  if (s.ptr && s.nwords < s.cap) *--s.ptr = w;
  ++s.nwords;
}

// rans64.h Rans64EncPut.  x / freq is a 64-by-32 division with x < 2^47 * freq after the
// renormalisation, i.e. a quotient below 2^47: a double-precision estimate (relative error
// ~2^-51, so off by at most one) corrected by the remainder gives the exact quotient without
// the long software division a GPU lane would otherwise run; the exact division remains as
// the never-taken guard, so the result does not depend on the estimate's accuracy.
RGBAC_HD inline void enc_put(EncState& s, uint32_t start, uint32_t freq) {
  uint64_t x = s.x;
  const uint64_t x_max = ((kL >> kPrecision) << 32) * freq;
  if (x >= x_max) {
    emit(s, (uint32_t)x);
    x >>= 32;
  }
  uint64_t q = (uint64_t)((double)x * (1.0 / (double)freq));
  int64_t r = (int64_t)(x - q * freq);
  if (r < 0) {
    --q;
    r += freq;
  } else if (r >= (int64_t)freq) {
    ++q;
    r -= freq;
  }
  if (r < 0 || r >= (int64_t)freq) {
    q = x / freq;
    r = (int64_t)(x - q * freq);
  }
  s.x = (q << kPrecision) + (uint64_t)r + start;
}

// rans_interface.cpp Rans64EncPutBits with nbits = 4
RGBAC_HD inline void enc_put_bits(EncState& s, uint32_t val) {
  uint64_t x = s.x;
  const uint64_t x_max = ((kL >> 16) << 32) * (uint64_t)(1u << (16 - kBypassBits));
  if (x >= x_max) {
    emit(s, (uint32_t)x);
    x >>= 32;
  }
  s.x = (x << kBypassBits) | val;
}

struct DecState {
  uint64_t x;
  const uint32_t* words;
  int32_t nwords;
  int32_t pos;
  int32_t err;
};

RGBAC_HD inline uint32_t dec_word(DecState& d) {
  if (d.pos >= d.nwords) {
    if (!d.err) d.err = kErrPastEnd;
    return 0;
  }
  return d.words[d.pos++];
}

// rans_interface.cpp Rans64DecGetBits with nbits = 4
RGBAC_HD inline uint32_t dec_get_bits(DecState& d) {
  uint64_t x = d.x;
  const uint32_t val = (uint32_t)(x & kMaxBypassVal);
  x >>= kBypassBits;
  if (x < kL) x = (x << 32) | dec_word(d);
  d.x = x;
  return val;
}

RGBAC_HD inline int32_t clamp_i32(int32_t v, int32_t lo, int32_t hi) {
  return v < lo ? lo : (v > hi ? hi : v);
}

}  // namespace detail

// Encodes sym[0..n) / idx[0..n) as one rANS stream: symbols last to first, per symbol the
// records rans.cpp's encode_into produces (CDF record, digit count, digits low to high) taken
// in reverse; words are stored backwards from ``end``, then the two state words.  With
// end == nullptr nothing is stored (count-only mode).  Returns the word count (<=
// chunk_bound(n)); the chunk occupies [end - count, end).  At most ``cap`` words are stored
// (the room the caller reserved below end, normally the count-only pass's result): a return
// value above cap means the stream was cut.  A bad CDF index or table row is clamped /
// skipped and recorded in *err (first code wins; err may not be null).
RGBAC_HD inline int64_t chunk_encode(const int32_t* sym, const int32_t* idx, int64_t n,
                                     const Tables& t, uint32_t* end, int64_t cap, int32_t* err) {
  detail::EncState s = {kL, end, cap, 0};
  for (int64_t i = n - 1; i >= 0; --i) {
    int32_t ci = idx[i];
    if (ci < 0 || ci >= t.ncdf) {
      if (!*err) *err = kErrIndex;
      ci = detail::clamp_i32(ci, 0, t.ncdf - 1);
    }
    const int32_t* cdf = t.cdfs + (int64_t)ci * t.stride;
    int32_t size = t.sizes[ci];
    if (size < 3 || size > t.stride) {
      if (!*err) *err = kErrCorrupt;
      size = detail::clamp_i32(size, 3, t.stride);
    }
    const int32_t max_value = size - 2;
    int64_t value = (int64_t)sym[i] - t.offsets[ci];
    uint32_t raw_val = 0;
    if (value < 0) {
      raw_val = (uint32_t)(-2 * value - 1);
      value = max_value;
    } else if (value >= max_value) {
      raw_val = (uint32_t)(2 * (value - max_value));
      value = max_value;
    }
    if (value == max_value) {
      int32_t n_bypass = 0;
      while (n_bypass < kMaxBypass && (raw_val >> (n_bypass * kBypassBits)) != 0) ++n_bypass;
      for (int32_t j = n_bypass - 1; j >= 0; --j)
        detail::enc_put_bits(s, (raw_val >> (j * kBypassBits)) & kMaxBypassVal);
      // the digit count: n_bypass <= 8 < 15, so rans.cpp's runs of 15 never occur
      detail::enc_put_bits(s, (uint32_t)n_bypass);
    }
    const uint32_t start = (uint32_t)cdf[value] & 0xFFFFu;
    const uint32_t freq = (uint32_t)(cdf[value + 1] - cdf[value]) & 0xFFFFu;
    if (freq == 0) {                       // not a CDF: nothing sane to emit, and no division
      if (!*err) *err = kErrCorrupt;
      continue;
    }
    detail::enc_put(s, start, freq);
  }
  detail::emit(s, (uint32_t)(s.x >> 32));
  detail::emit(s, (uint32_t)s.x);
  return s.nwords;
}

// Decodes n symbols of idx[0..n) from words[0..nwords) into out[0..n) (rans.cpp
// rgbac_rans_decode, every read bounded).  Returns 0 or the first error code; after an error
// the rest of out is filled with 0.
RGBAC_HD inline int32_t chunk_decode(const uint32_t* words, int32_t nwords, const int32_t* idx,
                                     int64_t n, const Tables& t, int32_t* out) {
  detail::DecState d = {0, words, nwords < 0 ? 0 : nwords, 0, kErrNone};
  const uint32_t lo = detail::dec_word(d), hi = detail::dec_word(d);
  d.x = (uint64_t)lo | ((uint64_t)hi << 32);
  const uint32_t mask = (1u << kPrecision) - 1;
  int64_t i = 0;
  for (; i < n && !d.err; ++i) {
    int32_t ci = idx[i];
    if (ci < 0 || ci >= t.ncdf) {
      d.err = kErrIndex;
      break;
    }
    const int32_t* cdf = t.cdfs + (int64_t)ci * t.stride;
    const int32_t size = t.sizes[ci];
    if (size < 3 || size > t.stride) {
      d.err = kErrCorrupt;
      break;
    }
    const int32_t max_value = size - 2;
    const int32_t cum = (int32_t)(d.x & mask);
    // upper_bound: first entry > cum, at most log2(stride) + 1 steps
    int32_t first = 0, len = size;
    while (len > 0) {
      const int32_t half = len >> 1;
      if (cdf[first + half] <= cum) {
        first += half + 1;
        len -= half + 1;
      } else {
        len = half;
      }
    }
    if (first == 0 || first == size) {
      d.err = kErrCorrupt;
      break;
    }
    const int32_t s = first - 1;
    const uint32_t start = (uint32_t)cdf[s], freq = (uint32_t)(cdf[s + 1] - cdf[s]);
    uint64_t x = d.x;
    x = freq * (x >> kPrecision) + (x & mask) - start;
    if (x < kL) x = (x << 32) | detail::dec_word(d);
    d.x = x;
    int32_t value = s;
    if (value == max_value) {
      uint32_t val = detail::dec_get_bits(d);
      int32_t n_bypass = (int32_t)val;
      // a count digit of 15 continues the count; any continuation exceeds 8 digits
      if (val == kMaxBypassVal) n_bypass += (int32_t)detail::dec_get_bits(d);
      if (n_bypass > kMaxBypass) {
        if (!d.err) d.err = kErrBypass;
        break;
      }
      uint32_t raw_val = 0;
      for (int32_t j = 0; j < n_bypass; ++j) raw_val |= detail::dec_get_bits(d) << (j * kBypassBits);
      const uint32_t mag = raw_val >> 1;
      const uint32_t v = (raw_val & 1) ? ~mag : mag + (uint32_t)max_value;   // -mag - 1 == ~mag
      value = (int32_t)v;
    }
    if (d.err) break;
    out[i] = (int32_t)((uint32_t)value + (uint32_t)t.offsets[ci]);
  }
  if (d.err)
    for (; i < n; ++i) out[i] = 0;
  return d.err;
}

}  // namespace rgbac_rans
#endif  // RGBAC_RANS_CHUNK_H_
