// fwd1024_forms.h -- the forms of stft1024_h256_fwd_kernel (stft1024.hip) and the choice between them.
//
// A form is a traits type: the kernel is instantiated once per form and reads every compile-time switch from it.
// FwdForm holds the defaults (the plain forward at hop 256), each named form overrides what differs.  pick_fwd1024()
// maps a call to a form id; the launcher's table turns the id into a kernel pointer and a launch shape, every field of
// it taken from the same type.  No HIP in here: tests/test_fwd1024_forms_cpu.py compiles the choice on the host.
#pragma once

namespace at_hip {
namespace fwd1024 {

// pass lengths of the reference's default bank at sr 44100 / n_fft 1024 in quads, one per nibble (band_bank.h).  The packed
// epilogue also hard-codes the feature row as 513 floats (its 1-KB block stream): the choice below asks for
// n_filters == 513 as well -- a 514..576-filter bank can have the same nine pass lengths
constexpr unsigned long long kDefaultBankQuads = 0x001111223ull;
constexpr int kDefaultBankPasses = 9;      // 513 filters: seven passes of walks, two of empty filters

struct FwdForm {
  static constexpr bool write_phase = false;   // the side output angle(X) per bin, (B*T, 513) floats
  static constexpr int mel = 0;      // 0 = spectrum only; 1 = spectrum + fused banded-filterbank features; 2 = features only.
  static constexpr int waves = 4;    // per workgroup; they share the LDS constant tables (twiddles are always staged there)
  // the FFT reads its twiddles from LDS at the point of use instead of holding 44 VGPRs, which buys a fourth wave per SIMD
  static constexpr bool lds_twiddles = false;
  // (mel != 0, channel-major features): number of passes whose outputs are kept for eight frames in registers and
  // written as 32 contiguous bytes per filter; 0 = every frame scatters 4-byte stores (each lane its own row of the
  // (B, N, T) tensor), which leaves partly written lines to be evicted and re-fetched.
  static constexpr int window_passes = 0;
  // (with mel == 2): besides the features, normalise(angle X) of every bin goes to p.phase with row stride p.phase_ld --
  // Compose(STFT + Polar) in one kernel, the complex spectrum never reaches HBM.
  static constexpr bool polar = false;
  // hop in 128-sample register slots (1, 2 = the reference's default hop 256, 4): the window slides hop_slots slots per
  // frame and hop_slots new segments are fetched.
  static constexpr int hop_slots = 2;
  // (row-major features of a one- or two-pass bank -- the 128-mel bank of the headline step): the passes are unrolled
  // and what a lane needs for them (its filter, where its walk starts, the walk's length) is read once per run instead
  // of once per pass and frame.
  static constexpr int hoisted_passes = 0;
  // (with hoisted_passes == 2): the two passes' walk lengths in quads as compile-time constants, contrast and power
  // fixed too (fixed_contrast, fixed_power2) -- the headline configuration (128 mel filters at 44.1 kHz: 8 and 2 quads,
  // log1p, |X|).  The generic epilogue spends more instructions on run-time switches (contrast mode, power, layout, loop
  // control: 112 scalar and 137 vector instructions per frame in the listing) than on the 20 multiply-adds of the walk
  // itself; with everything fixed both passes are straight-line code, their LDS reads batched and their sums independent.
  static constexpr int fixed_quads0 = 0, fixed_quads1 = 0;
  // the contrast of the fixed-length epilogue (1 = log1p, the headline; 2 = log of the clamped value: the log-mel of
  // BASELINE configs[3]; 0 = none) and |X|^2 instead of |X|
  static constexpr int fixed_contrast = 1;
  static constexpr bool fixed_power2 = false;
  // the spectrum leaves as ONE byte stream in 512-byte aligned blocks.  (B, T, 513) complex64 is contiguous and a wave
  // writes consecutive frames, but a row is 4104 bytes: row f starts 8 f bytes past a 128-byte line, every one of its
  // eight 512-byte stores straddles five lines and the Nyquist bin is a ninth, one-lane store.  With aligned_stores the
  // output COLUMNS of the FFT are rotated over the lanes by rot = (f 513) mod 64 (free: the last exchange reads through
  // the rotated index, fft512's out_lane), so that the lane number IS the position inside an aligned block of 64 bins:
  // lanes >= rot hold block j of the frame in register j, lanes < rot hold block j + 1 in register j, block 8 (the tail
  // of register 7, then the Nyquist bin on lane rot) is carried into the next frame's block 0.  Eight full, aligned
  // 512-byte stores per frame (a ninth every 64 frames), two selects per store, no masked store in the steady state.
  static constexpr bool aligned_stores = false;
  // those stores non-temporal.  tools/ubench/stream_pattern2.hip prices the pattern: rows 4.7 TB/s, aligned blocks 4.95,
  // aligned + nt 5.0-5.3 (profiles/r03a_*).
  static constexpr bool nontemporal = false;
  // (with lds_twiddles): bit 0 -- the two pass twiddle tables in registers, only the merge's W1024 rows from LDS
  // (HybridTwiddles); bit 1 -- the analysis window in registers.  Both trade LDS reads (the busiest unit of these
  // kernels) for VGPRs, i.e. for the fourth wave per SIMD.
  static constexpr int register_tables = 0;
  static constexpr bool persistent = false;   // workgroups take tiles of `waves` consecutive runs from a device counter
  // the fixed-length epilogue of a bank with many passes: their lengths in quads, one per nibble (band_bank.h), and
  // their number.  The launcher adds the packed per-lane descriptors to the dynamic LDS.
  static constexpr unsigned long long packed_quads = 0;
  static constexpr int packed_passes = 0;
};

template <class Form> constexpr int waves_per_simd() {
  return (Form::lds_twiddles && !Form::window_passes && !Form::register_tables) ? 4 : 3;
}
template <class Form> constexpr int packed_lds_bytes() {    // 16-byte rows of one word per pass, one row per lane
  return Form::packed_quads ? 64 * ((Form::packed_passes + 3) / 4 * 4) * (int)sizeof(int) : 0;
}

// plain forward: 4 waves per block, twiddles in registers (3 waves per SIMD).
struct Plain256 : FwdForm {};
struct Plain128 : FwdForm { static constexpr int hop_slots = 1; };
struct Plain512 : FwdForm { static constexpr int hop_slots = 4; };
struct PhasePlain256 : Plain256 { static constexpr bool write_phase = true; };
struct PhasePlain128 : Plain128 { static constexpr bool write_phase = true; };
struct PhasePlain512 : Plain512 { static constexpr bool write_phase = true; };
struct PlainAligned : FwdForm { static constexpr int waves = 8; static constexpr bool lds_twiddles = true, aligned_stores = true; };
struct PlainAlignedNt : PlainAligned { static constexpr bool nontemporal = true; };
struct PlainAlignedNtPersistent : PlainAlignedNt { static constexpr bool persistent = true; };
// fused: 8 waves share the band table and read their twiddles from a workgroup LDS copy, which frees 44 VGPRs for a
// 4th wave per SIMD to cover the epilogue's LDS round trips (4 % faster than the 3-wave form, A/B on one device).
struct GenericFeatures256 : FwdForm { static constexpr int mel = 2, waves = 8; static constexpr bool lds_twiddles = true; };
struct GenericFeatures128 : GenericFeatures256 { static constexpr int hop_slots = 1; };
struct GenericFeatures512 : GenericFeatures256 { static constexpr int hop_slots = 4; };
struct GenericSpectrum256 : GenericFeatures256 { static constexpr int mel = 1; };
struct GenericSpectrum128 : GenericFeatures128 { static constexpr int mel = 1; };
struct GenericSpectrum512 : GenericFeatures512 { static constexpr int mel = 1; };
struct PhaseGenericSpectrum256 : GenericSpectrum256 { static constexpr bool write_phase = true; };
struct PhaseGenericSpectrum128 : GenericSpectrum128 { static constexpr bool write_phase = true; };
struct PhaseGenericSpectrum512 : GenericSpectrum512 { static constexpr bool write_phase = true; };
struct ChannelMajor1 : GenericFeatures256 { static constexpr int window_passes = 1; };
struct ChannelMajor2 : GenericFeatures256 { static constexpr int window_passes = 2; };
struct Polar : GenericFeatures256 { static constexpr bool polar = true; };
struct Hoisted1Features : GenericFeatures256 { static constexpr int hoisted_passes = 1; };
struct Hoisted2Features : GenericFeatures256 { static constexpr int hoisted_passes = 2; };
struct Hoisted1Spectrum : Hoisted1Features { static constexpr int mel = 1; };
struct Hoisted2Spectrum : Hoisted2Features { static constexpr int mel = 1; };
// the fixed 8 + 2-quad epilogue of the 128-mel bank
struct FixedMel128Spectrum : Hoisted2Spectrum { static constexpr int fixed_quads0 = 8, fixed_quads1 = 2; };
struct FixedMel128SpectrumAligned : FixedMel128Spectrum { static constexpr bool aligned_stores = true; };
struct FixedMel128SpectrumAlignedNt : FixedMel128SpectrumAligned { static constexpr bool nontemporal = true; };
struct FixedMel128SpectrumAlignedNtPersistent : FixedMel128SpectrumAlignedNt { static constexpr bool persistent = true; };
struct FixedMel128Features8Waves : Hoisted2Features { static constexpr int fixed_quads0 = 8, fixed_quads1 = 2; };
// Features only (the spectrum never stored) is bound by the LDS and by instruction issue, not by HBM: with both
// pass-twiddle tables and the window in registers (30 fewer LDS reads per frame) at three waves per SIMD -- three 4-wave
// blocks per CU -- it runs 4 % faster than with four waves that read everything from LDS (0.642 -> 0.615 ms, same box,
// alternating runs).  The spectrum-storing forms did not move with any setting (fused 0.867 / 0.866 / 0.869 ms, plain
// 0.756 / 0.758 / 0.779): their waves wait on store issue, and the plain one loses its fifth and sixth wave.  5 waves
// per SIMD (10-wave blocks, 96 registers, 2 spilled): 0.65 -> 0.69 ms.
struct FixedMel128Features : FixedMel128Features8Waves { static constexpr int waves = 4, register_tables = 3; };
// the log-mel of BASELINE configs[3] (log contrast, |X|^2, features only)
struct LogPowerMel128 : FixedMel128Features { static constexpr int fixed_contrast = 2; static constexpr bool fixed_power2 = true; };
// MelSpectrogram (the reference's MFCC: |X|^2 on the 128-filter bank, no contrast, channel-major (.., N, T) output,
// spectrum never stored), its two results parked in the register windows.  4-wave blocks at three waves per SIMD (142
// registers); with the pass twiddles in registers as well (register_tables = 3) the two windows no longer fit and spill
// (0.75 ms against 0.72; the run-time-length epilogue: 0.755)
struct MelSpectrogramChannelMajor : FixedMel128Features8Waves {
  static constexpr int waves = 4, window_passes = 2, fixed_contrast = 0;
  static constexpr bool fixed_power2 = true;
};
// The reference's default bank -- Magnitude() at sr 44100: 404 non-empty filters of 513 in seven passes of 3, 2, 2, 1,
// 1, 1, 1 quads (and two of empty filters) -- with log1p and |X|, FEATURES ONLY (the README chain's forward): the
// packed fixed-length epilogue, 0.92 -> 0.78-0.84 ms per 1024 clips.  The spectrum-storing form keeps the generic
// epilogue: it is bound by the memory system's rate for one read and two write streams (~4.1 TB/s), and neither fewer
// instructions (-31 %) nor fewer write requests (115 -> 96 per frame) nor aligned spectrum blocks moved it
// (1.25-1.34 ms in every combination, same boxes: profiles/r04_default_bank_513.md).
struct PackedDefaultBankFeatures : GenericFeatures256 {
  static constexpr unsigned long long packed_quads = kDefaultBankQuads;
  static constexpr int packed_passes = kDefaultBankPasses;
};
// -DAT_DEV_SWITCHES builds only (round 5, energy): pass twiddles (1) / + window (3) in registers, three waves per SIMD
// in 4-wave blocks
struct DevFixedMel128SpectrumTables1 : FixedMel128SpectrumAlignedNt { static constexpr int waves = 4, register_tables = 1; };
struct DevFixedMel128SpectrumTables3 : FixedMel128SpectrumAlignedNt { static constexpr int waves = 4, register_tables = 3; };

}  // namespace fwd1024

// every form, in the order of the ids; the two dev forms last (only a -DAT_DEV_SWITCHES build instantiates them)
#define AT_FWD1024_FORMS(X)                                                                                          \
  X(Plain128) X(Plain256) X(Plain512) X(PhasePlain128) X(PhasePlain256) X(PhasePlain512)                             \
  X(PlainAligned) X(PlainAlignedNt) X(PlainAlignedNtPersistent)                                                      \
  X(GenericFeatures128) X(GenericFeatures256) X(GenericFeatures512)                                                  \
  X(GenericSpectrum128) X(GenericSpectrum256) X(GenericSpectrum512)                                                  \
  X(PhaseGenericSpectrum128) X(PhaseGenericSpectrum256) X(PhaseGenericSpectrum512)                                   \
  X(ChannelMajor1) X(ChannelMajor2) X(Polar)                                                                         \
  X(Hoisted1Features) X(Hoisted2Features) X(Hoisted1Spectrum) X(Hoisted2Spectrum)                                    \
  X(FixedMel128Spectrum) X(FixedMel128SpectrumAligned) X(FixedMel128SpectrumAlignedNt)                               \
  X(FixedMel128SpectrumAlignedNtPersistent) X(FixedMel128Features8Waves) X(FixedMel128Features)                      \
  X(LogPowerMel128) X(MelSpectrogramChannelMajor) X(PackedDefaultBankFeatures)
#define AT_FWD1024_DEV_FORMS(X) X(DevFixedMel128SpectrumTables1) X(DevFixedMel128SpectrumTables3)

enum Fwd1024Form {
  kFwd1024Rejected = -1,
#define X(F) kFwd##F,
  AT_FWD1024_FORMS(X) AT_FWD1024_DEV_FORMS(X)
#undef X
  kFwd1024Forms,
  kFwd1024ProductForms = kFwdDevFixedMel128SpectrumTables1
};

// What the choice depends on.  The dev_* fields come from the environment in a -DAT_DEV_SWITCHES build and are the
// constants below in the product library.
struct Fwd1024Call {
  int hop;
  bool spectrum, phase, polar, channel_major;   // outputs wanted: out, phase, PolarOut, (B, N, T) features
  bool bank;                                    // a fused epilogue; the bank's shape:
  int n_passes, n_filters;
  const int* pass_len;
  int contrast;                                 // 0 none, 1 log1p, 2 log, 3 log10
  bool power2;
  bool out_aligned_512, feat_aligned_16;        // the output pointers
  int epilogue;                                 // variant(kVarEpilogue): 1 = never a fixed-length epilogue
  int dev_stores = 2;                           // ACIDS_FWD_STORES: 0 rows, 1 aligned, 2 aligned non-temporal
  bool dev_persistent = false;                  // ACIDS_FWD_PW
  int dev_register_tables = 0;                  // ACIDS_FWD_HYB
  bool dev_no_register_tables = false;          // ACIDS_FWD_NOHYB
};

// One of a family's three forms by hop.
constexpr int at_hop(int hop, int f128, int f256, int f512) { return hop == 128 ? f128 : hop == 256 ? f256 : f512; }

// Ordered rules, first match wins, most specific first.  kFwd1024Rejected: no kernel takes the call.
inline int pick_fwd1024(const Fwd1024Call& c) {
  if (c.hop != 256 && c.hop != 128 && c.hop != 512) return kFwd1024Rejected;
  // at hop 128 / 512 the fused epilogue exists in its two plain forms (spectrum + features, features only); the
  // channel-major (MFCC) and Polar variants are built for the reference's hop 256
  if (c.hop != 256 && c.bank && (c.polar || c.channel_major)) return kFwd1024Rejected;
  if (c.polar && (!c.bank || c.spectrum)) return kFwd1024Rejected;
  const bool h256 = c.hop == 256;
  // Aligned stream stores for the two headline forms at the default hop: the plain forward and the fixed-length fused
  // epilogue.  Persistent workgroups measured slower than one long run per wave on the product kernels
  // (profiles/r04_launch_shape.md): a development variant.
  const bool aligned = c.dev_stores != 0 && h256 && c.spectrum && !c.phase && !c.polar && c.out_aligned_512;
  const bool nt = c.dev_stores == 2;
  if (!c.bank) {
    if (aligned && nt && c.dev_persistent) return kFwdPlainAlignedNtPersistent;
    if (aligned) return nt ? kFwdPlainAlignedNt : kFwdPlainAligned;
    return c.phase ? at_hop(c.hop, kFwdPhasePlain128, kFwdPhasePlain256, kFwdPhasePlain512)
                   : at_hop(c.hop, kFwdPlain128, kFwdPlain256, kFwdPlain512);
  }
  // the specialised epilogues: default hop, no phase or polar output, not switched off by the epilogue variant
  const bool special = h256 && !c.polar && !c.phase && c.epilogue == 0;
  const bool row_major = !c.channel_major;
  const bool mel128 = c.n_passes == 2 && c.pass_len[0] == 32 && c.pass_len[1] == 8;   // 128 mel filters at 44.1 kHz
  if (special && mel128 && row_major && c.contrast == 1 && !c.power2) {                // ... with log1p and |X|: the headline
    if (!c.spectrum) return c.dev_no_register_tables ? kFwdFixedMel128Features8Waves : kFwdFixedMel128Features;
    if (!aligned) return kFwdFixedMel128Spectrum;
    if (c.dev_register_tables == 1) return kFwdDevFixedMel128SpectrumTables1;
    if (c.dev_register_tables == 3) return kFwdDevFixedMel128SpectrumTables3;
    if (nt && c.dev_persistent) return kFwdFixedMel128SpectrumAlignedNtPersistent;
    return nt ? kFwdFixedMel128SpectrumAlignedNt : kFwdFixedMel128SpectrumAligned;
  }
  if (special && mel128 && row_major && !c.spectrum && c.contrast == 2 && c.power2) return kFwdLogPowerMel128;
  if (special && mel128 && !row_major && !c.spectrum && c.contrast == 0 && c.power2) return kFwdMelSpectrogramChannelMajor;
  if (special && row_major && !c.spectrum && c.contrast == 1 && !c.power2 && c.n_filters == 513 && c.feat_aligned_16 &&
      c.n_passes == fwd1024::kDefaultBankPasses) {
    bool same = true;
    for (int q = 0; q < c.n_passes; ++q)
      same = same && c.pass_len[q] == 4 * (int)((fwd1024::kDefaultBankQuads >> (4 * q)) & 15u);
    if (same) return kFwdPackedDefaultBankFeatures;
  }
  // row-major features of a one- / two-pass bank at the default hop: passes unrolled, lane constants hoisted
  if (h256 && !c.polar && !c.phase && row_major && c.n_passes <= 2) {
    if (c.n_passes == 1) return c.spectrum ? kFwdHoisted1Spectrum : kFwdHoisted1Features;
    return c.spectrum ? kFwdHoisted2Spectrum : kFwdHoisted2Features;
  }
  // the generic epilogue
  if (c.spectrum)
    return c.phase ? at_hop(c.hop, kFwdPhaseGenericSpectrum128, kFwdPhaseGenericSpectrum256, kFwdPhaseGenericSpectrum512)
                   : at_hop(c.hop, kFwdGenericSpectrum128, kFwdGenericSpectrum256, kFwdGenericSpectrum512);
  if (c.polar) return kFwdPolar;
  if (c.channel_major && c.n_passes == 1) return kFwdChannelMajor1;
  if (c.channel_major && c.n_passes == 2) return kFwdChannelMajor2;
  return at_hop(c.hop, kFwdGenericFeatures128, kFwdGenericFeatures256, kFwdGenericFeatures512);
}

}  // namespace at_hip
