"""Which frames share one 512-point register FFT at n_fft 128 / 256 / 512, restated for the CPU, the dispatch that
sends a call to those kernels, a float32 model of the packing, and the sweeps of test_clip_isolation_gpu.py.

At n_fft = 1024 / K (K = 8 / 4 / 2) the register kernels transform K frames at once and unmix them afterwards
(csrc/stft_small.hip, csrc/stft512.hip).  Every output of the shared transform carries rounding error proportional to
the LARGEST member of the group, and a NaN in one member reaches all of them.  The groups are therefore formed per
clip: group g of a clip holds its frames K g .. K g + K - 1, the clip's last group is filled with exact zeros, and a
frame's slot is its index in the clip mod K (`groups`).  Nothing outside a clip -- for pre-framed input: outside one
leading-index row of frames, a stream -- reaches that clip's output.  `launch_wide_groups` is what the kernels did
before (f = K g + r over all B T frames): the GPU tests fail on it, and test_shared_fft_cases_cpu.py shows which of
the swept shapes tell the two apart.

The arithmetic follows csrc/capi.hip (at_stft_forward, at_istft, at_irfft_frames_streams, at_stft_mel_forward),
csrc/stft512.hip (launch_stft512_fwd, launch_stft512_mel, launch_irfft512_frames) and csrc/stft_small.hip
(launch_stft_small_fwd, launch_irfft_small_frames), with units_per_block of csrc/run_plan.h."""
import numpy as np

K_OF = {128: 8, 256: 4, 512: 2}       # frames per shared transform
WS = 4                                # waves per workgroup of the group kernels (stft_small.hip WS, stft512.hip W5)
MAX_BLOCKS = 256 * 8


def cdiv(a, b):
    return -(-a // b)


# ---- dispatch ---------------------------------------------------------------------------------------------------------
def forward_kernel(n_fft, hop, center=True, phase=False, L=1 << 20, clip_stride_odd=False, x_aligned=True,
                   out_aligned=True, frame_kernels=False):
    """at_stft_forward / launch_stft512_fwd (windows are 8-byte aligned in every module)."""
    if n_fft in (128, 256):
        return "stft_small_fwd_kernel<%d>" % K_OF[n_fft]
    if n_fft == 512:
        sliding = (center and hop == 128 and not phase and L >= 512 and not clip_stride_odd and x_aligned and out_aligned
                   and not frame_kernels)
        return "stft512_run_fwd_kernel" if sliding else "stft512_fwd_kernel"
    return "other"


def forward_reason(n_fft, hop, center=True, phase=False, L=1 << 20, clip_stride_odd=False, x_aligned=True,
                   out_aligned=True, frame_kernels=False):
    """The conditions of launch_stft512_fwd that keep a call off the sliding kernel."""
    r = set()
    if n_fft == 512:
        if hop != 128:
            r.add("hop_not_128")
        if not center:
            r.add("center_false")
        if phase:
            r.add("phase_output")
        if L < 512:
            r.add("L_lt_512")
        if clip_stride_odd:
            r.add("odd_clip_stride")
        if not x_aligned:
            r.add("unaligned_input")
        if not out_aligned:
            r.add("unaligned_output")
        if frame_kernels:
            r.add("variant_frame_kernels")
    return r


FWD512_REASONS = {"hop_not_128", "center_false", "phase_output", "L_lt_512", "odd_clip_stride", "unaligned_input",
                  "unaligned_output", "variant_frame_kernels"}


def istft_kernel(n_fft, hop, env=True):
    """at_istft: the frames kernel in front of the overlap-add gather, or the fused n_fft-512 kernel."""
    if n_fft in (128, 256):
        return "irfft_small_frames_kernel<%d>" % K_OF[n_fft]
    if n_fft == 512:
        return "istft512_ola_kernel" if (hop in (64, 128, 256) and env) else "irfft512_frames_kernel"
    return "other"


def irfft_frames_kernel(n_fft):
    """at_irfft_frames / at_irfft_frames_streams."""
    if n_fft in (128, 256):
        return "irfft_small_frames_kernel<%d>" % K_OF[n_fft]
    return "irfft512_frames_kernel" if n_fft == 512 else "other"


def mel_kernel(n_fft, want_spectrum=False):
    """at_stft_mel_forward, features only."""
    return "stft512_mel_kernel" if (n_fft == 512 and not want_spectrum) else "other"


# ---- grouping ---------------------------------------------------------------------------------------------------------
def groups(B, T, K):
    """Per clip: [[(b, t) or None] * K] in launch order; None is a slot filled with exact zeros."""
    out = []
    for b in range(B):
        for g in range(cdiv(T, K)):
            out.append([(b, K * g + r) if K * g + r < T else None for r in range(K)])
    return out


def launch_wide_groups(B, T, K):
    """The grouping before: f = K g + r over the B T frames of the launch."""
    out = []
    for g in range(cdiv(B * T, K)):
        out.append([divmod(K * g + r, T) if K * g + r < B * T else None for r in range(K)])
    return out


def mates(grouping, b, t):
    """The frames that share a transform with frame t of clip b (itself included)."""
    for grp in grouping:
        if (b, t) in grp:
            return {m for m in grp if m is not None}
    raise KeyError((b, t))


def clips_in_group(grp):
    return {m[0] for m in grp if m is not None}


def groups_per_block(ngroups):
    """units_per_block (run_plan.h): whole rounds of the workgroup's WS waves, 2048 workgroups at most."""
    gpb = cdiv(cdiv(ngroups, MAX_BLOCKS), WS) * WS
    return max(gpb, WS)


def mel_pairs_per_wave(B, T, v=0):
    """launch_stft512_mel: frame pairs per wave over the B * ceil(T / 2) pairs, at least 4 (AT_VARIANT_ROW_RUN = v)."""
    pairs = B * cdiv(T, 2)
    return min(v, max(pairs, 1)) if v > 0 else max(4, cdiv(pairs, MAX_BLOCKS * WS))


def extra_transform_work(T, K):
    """What zero-filling each clip's last group costs: ceil(T / K) K / T - 1."""
    return cdiv(T, K) * K / T - 1.0


# ---- geometry classes -------------------------------------------------------------------------------------------------
def geometry(B, T, K, tested=()):
    """Classes of a launch of B clips of T frames; `tested`: the clips compared against a batch of one."""
    c = {"rem_%d" % (T % K)}
    if T < K:
        c.add("T_lt_K_%d" % T)
    wide = launch_wide_groups(B, T, K)
    if max(len(clips_in_group(g)) for g in wide) >= 3:
        c.add("wide_group_holds_3_clips")
    if any(len(clips_in_group(g)) >= 2 for g in wide):
        c.add("wide_group_straddles")
    if (B * T) % K:
        c.add("last_group_partial")
    for b in tested:
        c.add("clip_first" if b == 0 else "clip_last" if b == B - 1 else "clip_middle")
    if groups_per_block(B * cdiv(T, K)) > WS:
        c.add("block_takes_more_than_WS_groups")
    assert all(len(clips_in_group(g)) == 1 for g in groups(B, T, K))
    return c


def geometry_classes(K):
    c = {"rem_%d" % r for r in range(K)} | {"T_lt_K_%d" % t for t in (1, 2, 3, 5, 7) if t < K}
    c |= {"wide_group_straddles", "last_group_partial", "clip_first", "clip_middle", "clip_last",
          "block_takes_more_than_WS_groups"}
    if K > 2:
        c.add("wide_group_holds_3_clips")     # K = 2: a pair holds two clips at most
    return c


def tested_clips(B):
    return sorted({0, B // 2, B - 1})


# ---- the sweeps -------------------------------------------------------------------------------------------------------
B_SWEEP = 5
B_LARGE = 4100          # two groups per clip: 8200 groups > 2048 workgroups x WS


def hops_of(n_fft):
    """n/4, n/8, n/2 and one hop that does not divide n_fft."""
    return [n_fft // 4, n_fft // 8, n_fft // 2, n_fft // 4 + 8]


def T_sweep(K):
    """Every remainder mod K twice over, and every T below K."""
    return list(range(1, 2 * K + 2))


def center_shape(n_fft, T, hop=None):
    """(hop, L) of a center=True call with T frames: T = 1 + L // hop and L > n_fft / 2 (reflect padding)."""
    if hop is None or hop * (T - 1) + 4 <= n_fft // 2:
        hop = n_fft // 2 if T >= 2 else n_fft
    L = hop * (T - 1) + (4 if T >= 2 else n_fft // 2 + 4)
    assert 1 + L // hop == T and L > n_fft // 2, (n_fft, T, hop, L)
    return hop, L


def forward_cases(n_fft):
    """[(B, T, hop, center, L)]: every T of the sweep framed by torch.stft's rule (center=True) and as an explicit
    center=False view, every hop at two lengths, and one large launch."""
    K = K_OF[n_fft]
    cases = []
    for T in T_sweep(K):
        hop, L = center_shape(n_fft, T, hops_of(n_fft)[T % 4])
        cases.append((B_SWEEP, T, hop, True, L))
        hop = hops_of(n_fft)[(T + 1) % 4]
        cases.append((B_SWEEP, T, hop, False, hop * (T - 1) + n_fft))
    for hop in hops_of(n_fft):
        for T in (2 * K + 1, 2 * K + 3):
            h, L = center_shape(n_fft, T, hop)
            cases.append((B_SWEEP, T, h, True, L))
    T = K + 1
    hop = n_fft // 2
    cases.append((B_LARGE, T, hop, False, hop * (T - 1) + n_fft))
    return cases


def inverse_cases(n_fft):
    """[(B, T, hop)] of at_istft: T from 2 (one frame of an even size has no output), every hop."""
    K = K_OF[n_fft]
    cases = [(B_SWEEP, T, hops_of(n_fft)[T % 4]) for T in T_sweep(K) if T >= 2]
    cases += [(B_SWEEP, T, hop) for hop in hops_of(n_fft) for T in (2 * K + 1, 2 * K + 3)]
    if n_fft == 512:
        # hops n/8, n/4, n/2 take the fused kernel (a control): every T once more at the hop that does not
        cases += [(B_SWEEP, T, hops_of(512)[3]) for T in T_sweep(K) if T >= 2]
        cases.append((B_LARGE, K + 1, hops_of(512)[3]))
    else:
        cases.append((B_LARGE, K + 1, n_fft // 2))
    return cases


def frames_cases(n_fft):
    """[(S, n)] of pre-framed calls (RealtimeSTFT / RealtimeDGT, ops.irfft_frames): S streams of n frames."""
    K = K_OF[n_fft]
    return [(B_SWEEP, n) for n in sorted(set(T_sweep(K)) | {1, 5})] + [(B_LARGE, K + 1)]


MEL_ROW_RUNS = (0, 1, 3)          # AT_VARIANT_ROW_RUN: the default plan (4 pairs per wave), 1 and 3 pairs per wave


def mel_cases():
    """[(B, T, hop, L)] at n_fft 512."""
    out = []
    for T in T_sweep(2) + [9, 12]:
        hop, L = center_shape(512, T, 128)
        out.append((B_SWEEP, T, hop, L))
    return out


def swept_geometry(n_fft, kind):
    K = K_OF[n_fft]
    hit = set()
    if kind == "forward":
        # the frames-per-transform kernel only: the sliding n_fft-512 kernel (a control) walks one clip per wave
        shapes = [(B, T) for B, T, hop, center, L in forward_cases(n_fft)
                  if forward_kernel(n_fft, hop, center, L=L) != "stft512_run_fwd_kernel"]
    elif kind == "inverse":
        shapes = [(B, T) for B, T, hop in inverse_cases(n_fft) if istft_kernel(n_fft, hop) != "istft512_ola_kernel"]
    elif kind == "frames":
        shapes = frames_cases(n_fft)
    else:
        shapes = [(B, T) for B, T, _, _ in mel_cases()]
    for B, T in shapes:
        hit |= geometry(B, T, K, tested_clips(B))
    return hit


# ---- the per-clip metric ------------------------------------------------------------------------------------------------
def rel_max_per_clip(a, b):
    """max|a - b| / max|b| of every clip (leading index) on its own: [B] floats.  conftest.rel_max divides by the
    maximum of the whole tensor, behind which a wrong quiet clip hides next to a loud one."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    a, b = a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1)
    den = np.abs(b).max(axis=1)
    assert (den > 0).all(), "a clip whose reference is zero has no relative error"
    return np.abs(a - b).max(axis=1) / den


# ---- float32 model of the packing ---------------------------------------------------------------------------------------
def fft_c64(y):
    """Radix-2 decimation-in-time FFT kept in complex64 at every step."""
    n = len(y)
    if n == 1:
        return y.astype(np.complex64)
    e, o = fft_c64(y[0::2]), fft_c64(y[1::2])
    w = np.exp(-2j * np.pi * np.arange(n // 2) / n).astype(np.complex64)
    t = (w * o).astype(np.complex64)
    return np.concatenate([(e + t).astype(np.complex64), (e - t).astype(np.complex64)])


def packed_rfft_model(frames):
    """K real frames of N = 1024 / K float32 samples through ONE 512-point complex64 FFT, as stft_small.hip's header has
    it: y[K n + r] = a_r[n] with a_r[n] = x_r[2n] + i x_r[2n + 1]; Y[k + M q] = sum_r W512^(r k) W_K^(r q) A_r[k]; a
    K-point inverse DFT over q and the twiddle give A_r; the real split gives X_r[0 .. M].  Returns (K, M + 1) complex64."""
    frames = np.asarray(frames, dtype=np.float32)
    K, N = frames.shape
    M = N // 2
    assert K * M == 512
    a = (frames[:, 0::2] + 1j * frames[:, 1::2]).astype(np.complex64)           # (K, M)
    y = np.zeros(512, dtype=np.complex64)
    for r in range(K):
        y[r::K] = a[r]
    Y = fft_c64(y).reshape(K, M)                                                  # Y[q, k] = Y[k + M q]
    k = np.arange(M)
    out = np.zeros((K, M + 1), dtype=np.complex64)
    for r in range(K):
        acc = np.zeros(M, dtype=np.complex64)
        for q in range(K):
            acc = (acc + Y[q] * np.complex64(np.exp(2j * np.pi * r * q / K))).astype(np.complex64)
        A = (acc * np.exp(2j * np.pi * r * k / 512).astype(np.complex64) * np.float32(1.0 / K)).astype(np.complex64)
        Am = np.conj(A[(M - k) % M])
        wn = np.exp(-2j * np.pi * k / N).astype(np.complex64)
        X = (np.complex64(0.5) * ((A + Am) - 1j * wn * (A - Am))).astype(np.complex64)
        out[r, :M] = X
        out[r, M] = np.float32(A[0].real - A[0].imag)
    return out


def model_error(K, ratio, seed=0, zeros=False):
    """Error of one quiet frame (slot 0 .. K - 1 in turn, the worst) whose group mates are `ratio` times louder (or
    exact zeros), against a float64 rFFT, relative to the quiet frame's own maximum."""
    N = 1024 // K
    rng = np.random.default_rng(seed)
    worst = 0.0
    for slot in range(K):
        fr = (rng.standard_normal((K, N)) * (0.0 if zeros else ratio)).astype(np.float32)
        fr[slot] = rng.standard_normal(N).astype(np.float32)
        ref = np.fft.rfft(fr[slot].astype(np.float64))
        got = packed_rfft_model(fr)[slot]
        worst = max(worst, float(np.abs(got - ref).max() / np.abs(ref).max()))
    return worst
