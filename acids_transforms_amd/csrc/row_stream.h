// row_stream.h -- how the sliding-window forward kernels write their spectrum: the (B, T, F) tensor, F = n_fft / 2 + 1 =
// 64 NB + 1 complex bins a row, leaves as ONE stream of 512-byte aligned blocks (64 lanes x 8 bytes: four whole 128-byte
// lines per store instruction), whatever the row length.  Used by stft512_run_fwd_kernel (NB = 4), stft2048_run_fwd_kernel
// (16) and stft4096_run_fwd_kernel (32), whose device code is instruction for instruction what it was with the state
// machine written out in each (tools/isa_same.py); and the units of a run, which all four sizes take from here.
// The aligned forms of stft1024_h256_fwd_kernel (NB = 8) keep their own copy of the same state machine: on this struct
// six of that kernel's forms compile to a different run start (a frame peeled, two or three instructions fewer, two
// registers more in two forms), and in the same-process A/B against the parent build the step's median came out above
// the parent's by more than the spread of two copies of the parent (profiles/row_stream.md).  The struct is not bent
// for one size's register allocation.
//
// A wave walks a run of consecutive frames of one clip; the rows of a (B, T, F) tensor are contiguous, so the run's
// output is the elements [e0, e0 + n F) of the stream, e0 = (b T + t0) F.  A row is 8 F = 512 NB + 8 bytes: row g (its
// global frame index) starts 8 (g mod 64) bytes past a block boundary, so bin k of the row belongs in lane
// (k + rot) mod 64 of its block, rot = (g F) mod 64 = (rot of the row before + 1) mod 64.  The transform cores deliver
// that order: their output columns are rotated over the lanes, this lane holds bins col + 64 m, col = (lane - rot) & 63,
// in register m (the FFT's last exchange writes rotated addresses; twiddles and mirror lane follow the column).  Then
//   lanes >= rot:  register m sits in block m of the frame,
//   lanes <  rot:  register m sits in block m + 1; block 0 takes what the frame before left over -- `carry`: the tail of
//                  its last register (lanes < its rot) and its Nyquist bin (lane = its rot, the lane whose column is 0),
// and the frame's own tail and Nyquist bin are carried on: NB full-block stores per frame.  The frame with rot = 63
// fills its last block exactly (63 tail bins and the Nyquist bin): an NB + 1st store, every 64 frames, and an empty carry.
// The run's first block belongs to the run before it up to lane rot (`head`: those lanes are masked once), its last
// block to the next run -- or the next clip -- from lane rot on (end()): adjacent runs tile the stream, no element is
// written twice and none is skipped, which is what tests/row_stream_main.cpp checks for every start and these lengths.
//
// The store is a stateless functor type (n_fft 1024 has a non-temporal and a plain form), the value type a template
// parameter and there is no HIP include, the way stream_source.h is written: the host program instantiates the struct
// with integers and a recording store.
#pragma once

#ifdef __HIPCC__
#define AT_HD __host__ __device__
#else
#define AT_HD
#endif

namespace at_hip {

struct StoreNontemporal {      // written once, not read by this launch: past the caches
  template <typename V>
  AT_HD void operator()(V* dst, V val) const { __builtin_nontemporal_store(val, dst); }
};
struct StorePlain {
  template <typename V>
  AT_HD void operator()(V* dst, V val) const { *dst = val; }
};

template <int NB, typename V, typename PUT = StoreNontemporal>
struct RowStream {
  V* sp;        // this lane's slot in block 0 of the current frame
  V carry;      // what the previous frame left over: lanes < rot - 1 its last register's tail, lane rot - 1 its Nyquist bin
  int rot;      // column rotation of the current frame (wave-uniform); the cores want col = (lane - rot) & 63
  bool head;    // nothing emitted yet

  // X: the whole tensor (512-byte aligned); e0: the run's first element
  AT_HD void begin(V* X, long long e0, int lane) {
    rot = (int)(e0 & 63);
    sp = X + (e0 - rot) + lane;
    carry = V{};
    head = true;
  }

  // one frame: z[m] = bin col + 64 m, nyq = bin 64 NB (meaningful on the lane whose column is 0, lane rot)
  AT_HD void emit(const V (&z)[NB], V nyq, int lane) {
    const bool lo = lane < rot;
    const V s0 = lo ? carry : z[0];
    if (head) {
      if (!lo) PUT()(sp, s0);
      head = false;
    } else {
      PUT()(sp, s0);
    }
#pragma unroll
    for (int j = 1; j < NB; ++j) PUT()(sp + 64 * j, lo ? z[j - 1] : z[j]);
    carry = lo ? z[NB - 1] : nyq;
    if (rot == 63) {           // the frame ends exactly on a block boundary
      PUT()(sp + 64 * NB, carry);
      sp += 64 * NB + 64;
      rot = 0;
    } else {
      sp += 64 * NB;
      ++rot;
    }
  }

  // the run's last block: the next run (or clip) owns the rest of it
  AT_HD void end(int lane) const {
    if (lane < rot) PUT()(sp, carry);
  }
};

// The cut of a launch into runs, one wave per run: wave `run` takes run r = run - b runs_per_clip of clip
// b = run / runs_per_clip (a launch is whole workgroups: b >= B is a wave with nothing to do, and so is an empty run).
// The units [u0, u1) of run r of a clip's `units` (frames; frame pairs at n_fft 512) in runs of units_per_run, the last
// one shorter; false: none.
AT_HD inline bool run_units(long long r, long long units_per_run, long long units, long long& u0, long long& u1) {
  u0 = r * units_per_run;
  u1 = u0 + units_per_run;
  if (u1 > units) u1 = units;
  return u0 < u1;
}

}  // namespace at_hip
