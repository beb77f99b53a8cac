"""Which form of stft1024_h256_fwd_kernel a call gets (csrc/fwd1024_forms.h: pick_fwd1024), checked on the host.

Results cannot tell the forms apart -- they agree to 1e-5 -- so a slip in the choice only costs speed.  The expected
forms below restate README.md ("The forms of the n_fft-1024 forward") and the comments of the header; nothing here is
derived from the rules themselves.  tests/fwd1024_forms_main.cpp is compiled with the host compiler of the ROCm
toolchain that the library's Makefile needs anyway.
"""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "acids_transforms_amd", "csrc")

# bank shapes: n_filters, pass lengths in bins.  128 mel filters at 44.1 kHz walk 8 and 2 quads; the reference's default
# bank has 513 filters in seven passes of 3, 2, 2, 1, 1, 1, 1 quads and two passes of empty filters.
DEFAULT_LENS = (12, 8, 8, 4, 4, 4, 4, 0, 0)
BANKS = {
    "mel128": (128, (32, 8)),
    "one_pass": (64, (32,)),
    "two_pass": (128, (32, 12)),
    "two_pass_swapped": (128, (8, 32)),
    "one_pass_short": (64, (8,)),
    "no_pass": (0, ()),              # the launcher sends a bank without passes where it sends a two-pass one
    "default513": (513, DEFAULT_LENS),
    "default514": (514, DEFAULT_LENS),
    "nine_other": (513, (12, 8, 8, 4, 4, 4, 8, 0, 0)),
    "three_pass": (160, (16, 8, 4)),
}
BANK_NAMES = list(BANKS)
CONTRAST = {None: 0, "log1p": 1, "log": 2, "log10": 3}
FIELDS = ["hop", "spectrum", "phase", "polar", "channel_major", "bank", "contrast", "power2", "out_aligned_512",
          "feat_aligned_16", "epilogue", "dev_stores", "dev_persistent", "dev_register_tables", "dev_no_register_tables"]
PRODUCT = dict(dev_stores=2, dev_persistent=0, dev_register_tables=0, dev_no_register_tables=0)
MEMBERS = ["product", "hop_slots", "write_phase", "polar", "mel", "window_passes", "hoisted_passes", "fixed_quads0",
           "fixed_quads1", "fixed_contrast", "fixed_power2", "aligned_stores", "nontemporal", "persistent", "packed_passes",
           "packed_quads"]


def _host_compiler():
    roots = [os.environ.get("ROCM_PATH"), os.environ.get("ROCM_HOME"), "/opt/rocm"]
    for root in filter(None, roots):
        for sub in ("llvm/bin/clang++", "lib/llvm/bin/clang++", "bin/amdclang++"):
            if os.path.exists(os.path.join(root, sub)):
                return os.path.join(root, sub)
    pytest.fail("no host compiler of the ROCm toolchain found under %s" % [r for r in roots if r])


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fwd1024_forms") / "fwd1024_forms")
    subprocess.run([_host_compiler(), "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tests", "fwd1024_forms_main.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def forms(prog):
    """name and members of every form, by id"""
    rows = [l.split() for l in subprocess.run([prog, "--forms"], check=True, capture_output=True, text=True).stdout.splitlines()]
    assert [int(r[0]) for r in rows] == list(range(len(rows)))
    table = {m: np.array([int(r[2 + i]) for r in rows], dtype=np.uint64 if m == "packed_quads" else np.int64)
             for i, m in enumerate(MEMBERS)}
    return [r[1] for r in rows], table


def pick(prog, calls):
    """form ids of an (n, 15) array of calls, columns as FIELDS (bank: index into BANK_NAMES, -1 none)"""
    rec = np.zeros((len(calls), 16), dtype=np.int16)
    rec[:, :15] = calls
    shapes = ["%d:%s" % (BANKS[b][0], ",".join(map(str, BANKS[b][1]))) for b in BANK_NAMES]
    out = subprocess.run([prog] + shapes, input=rec.tobytes(), check=True, capture_output=True).stdout
    ids = np.array(out.split(), dtype=np.int64)
    assert len(ids) == len(calls)
    return ids


def one(prog, forms, **kw):
    call = dict(hop=256, spectrum=1, phase=0, polar=0, channel_major=0, bank=None, contrast="log1p", power2=0,
                out_aligned_512=1, feat_aligned_16=1, epilogue=0, **PRODUCT)
    call.update(kw)
    call["bank"] = -1 if call["bank"] is None else BANK_NAMES.index(call["bank"])
    call["contrast"] = CONTRAST[call["contrast"]]
    f = int(pick(prog, np.array([[call[k] for k in FIELDS]]))[0])
    return "rejected" if f < 0 else forms[0][f]


def test_named_configurations(prog, forms):
    def fused(n_mels, contrast, power, cm, spec, **kw):     # the arguments of FUSED_FORMS in tests/test_run_plans_gpu.py
        return one(prog, forms, bank="mel128" if n_mels else "default513", contrast=contrast, power2=int(power == 2),
                   channel_major=int(cm), spectrum=int(spec), **kw)
    assert fused(128, "log1p", 1, False, True) == "FixedMel128SpectrumAlignedNt"                # mel128_fixed
    assert fused(128, "log1p", 1, False, False) == "FixedMel128Features"                         # mel128_fixed_features
    assert fused(128, "log1p", 1, False, True, epilogue=1) == "Hoisted2Spectrum"                 # mel128_generic
    assert fused(128, None, 2, True, False) == "MelSpectrogramChannelMajor"                      # mfcc_channel_major
    assert fused(128, "log", 2, False, False) == "LogPowerMel128"                                # config3_logmel
    assert fused(None, "log1p", 1, False, False) == "PackedDefaultBankFeatures"                  # default_bank_features
    # epilogue = 1: the hoisted two-pass form, never a fixed one -- whatever else the call asks for
    assert fused(128, "log1p", 1, False, False, epilogue=1) == "Hoisted2Features"
    assert fused(128, "log", 2, False, False, epilogue=1) == "Hoisted2Features"
    assert fused(None, "log1p", 1, False, False, epilogue=1) == "GenericFeatures256"
    # the packed epilogue streams 16-byte aligned blocks of a 513-float row
    assert fused(None, "log1p", 1, False, False, feat_aligned_16=0) == "GenericFeatures256"
    assert one(prog, forms, bank="default514", spectrum=0) == "GenericFeatures256"
    assert fused(None, "log1p", 1, False, True) == "GenericSpectrum256"       # spectrum + default bank: generic (memory bound)
    # the headline bank with log contrast and |X|: no fixed form has that pair
    assert fused(128, "log", 1, False, False) == "Hoisted2Features"
    assert fused(128, "log", 1, False, True) == "Hoisted2Spectrum"
    # the aligned block stream needs a 512-byte aligned spectrum
    assert fused(128, "log1p", 1, False, True, out_aligned_512=0) == "FixedMel128Spectrum"
    assert one(prog, forms) == "PlainAlignedNt"
    assert one(prog, forms, out_aligned_512=0) == "Plain256"
    assert one(prog, forms, phase=1) == "PhasePlain256"
    # the other hops: plain and generic fused forms only
    for hop in (128, 512):
        assert fused(128, "log1p", 1, False, True, hop=hop) == "GenericSpectrum%d" % hop
        assert fused(128, "log1p", 1, False, False, hop=hop) == "GenericFeatures%d" % hop
        assert fused(128, "log1p", 1, False, True, phase=1, hop=hop) == "PhaseGenericSpectrum%d" % hop
        assert one(prog, forms, hop=hop) == "Plain%d" % hop
        assert one(prog, forms, bank="mel128", spectrum=0, polar=1, hop=hop) == "rejected"
        assert one(prog, forms, bank="mel128", spectrum=0, channel_major=1, hop=hop) == "rejected"
    assert one(prog, forms, bank="mel128", spectrum=0, polar=1) == "Polar"
    assert one(prog, forms, bank="mel128", spectrum=1, polar=1) == "rejected"
    assert one(prog, forms, spectrum=0, polar=1) == "rejected"                 # Polar is an epilogue: it needs a bank
    assert one(prog, forms, hop=64) == "rejected"
    assert one(prog, forms, bank="one_pass", spectrum=0, channel_major=1, contrast=None) == "ChannelMajor1"
    assert one(prog, forms, bank="two_pass", spectrum=0, channel_major=1, contrast=None) == "ChannelMajor2"
    assert one(prog, forms, bank="three_pass", spectrum=0, channel_major=1, contrast=None) == "GenericFeatures256"
    # both pass lengths make the 128-mel bank, not one of them
    assert one(prog, forms, bank="two_pass_swapped") == "Hoisted2Spectrum"
    assert one(prog, forms, bank="two_pass") == "Hoisted2Spectrum"
    assert one(prog, forms, bank="one_pass_short", spectrum=0) == "Hoisted1Features"


def test_every_call_of_the_grid(prog, forms):
    names, m = forms
    axes = dict(hop=[128, 256, 512], spectrum=[0, 1], phase=[0, 1], polar=[0, 1], channel_major=[0, 1],
                bank=list(range(-1, len(BANK_NAMES))), contrast=[0, 1, 2, 3], power2=[0, 1], out_aligned_512=[0, 1],
                feat_aligned_16=[0, 1], epilogue=[0, 1], dev_stores=[0, 1, 2], dev_persistent=[0, 1],
                dev_register_tables=[0, 1, 3], dev_no_register_tables=[0, 1])
    assert list(axes) == FIELDS
    grid = np.stack(np.meshgrid(*[np.array(v, dtype=np.int16) for v in axes.values()], indexing="ij"), -1).reshape(-1, len(FIELDS))
    assert len(grid) == 3 * 2 ** 10 * (1 + len(BANKS)) * 4 * 3 * 3
    ids = pick(prog, grid)
    c = {k: grid[:, i].astype(np.int64) for i, k in enumerate(FIELDS)}
    has_bank = c["bank"] >= 0
    n_passes = np.array([0] + [len(BANKS[b][1]) for b in BANK_NAMES])[c["bank"] + 1]

    # rejected: exactly the calls no kernel was built for
    rejected = ((c["hop"] != 256) & has_bank & ((c["polar"] | c["channel_major"]) == 1)) | \
               ((c["polar"] == 1) & (~has_bank | (c["spectrum"] == 1)))
    assert np.array_equal(ids < 0, rejected)
    ok = ids >= 0
    f = ids[ok]
    c = {k: v[ok] for k, v in c.items()}
    has_bank, n_passes = has_bank[ok], n_passes[ok]
    bank_is = {b: c["bank"] == i for i, b in enumerate(BANK_NAMES)}
    F = {k: v[f] for k, v in m.items()}

    def implies(a, b):
        bad = a & ~b
        assert not bad.any(), (names[f[bad][0]], {k: int(v[bad][0]) for k, v in c.items()})

    # the form's members agree with the call
    assert np.array_equal(F["hop_slots"] * 128, c["hop"])
    assert np.array_equal(F["polar"], c["polar"])
    assert np.array_equal(F["mel"] == 0, ~has_bank)
    assert np.array_equal(F["mel"] != 2, (c["spectrum"] == 1) | ~has_bank)
    # the phase rows go with the spectrum: a fused call that stores no spectrum writes no angle(X) rows either
    assert np.array_equal(F["write_phase"] == 1, (c["phase"] == 1) & ((c["spectrum"] == 1) | ~has_bank))
    # register windows: channel-major calls only, one per pass
    win = F["window_passes"] > 0
    implies(win, (c["channel_major"] == 1) & (F["window_passes"] == n_passes) & (c["spectrum"] == 0))
    # hoisted lane constants: one- and two-pass banks, row-major unless the results wait in the register windows
    implies(F["hoisted_passes"] > 0, has_bank & (F["hoisted_passes"] == np.where(n_passes == 0, 2, n_passes)) &
            (win | (c["channel_major"] == 0)))
    # fixed lengths only where the bank has them, with the contrast and power the form fixes
    fixed = F["fixed_quads0"] > 0
    implies(fixed, bank_is["mel128"] & (F["fixed_quads0"] == 8) & (F["fixed_quads1"] == 2) & (F["hoisted_passes"] == 2))
    implies(fixed, (F["fixed_contrast"] == c["contrast"]) & (F["fixed_power2"] == c["power2"]))
    packed = F["packed_passes"] > 0
    quads = sum(q << (4 * i) for i, q in enumerate(l // 4 for l in DEFAULT_LENS))
    implies(packed, bank_is["default513"] & (F["packed_passes"] == 9) & (F["packed_quads"] == quads))
    implies(packed, (c["contrast"] == 1) & (c["power2"] == 0) & (c["feat_aligned_16"] == 1) & (c["spectrum"] == 0))
    implies(fixed | packed, (c["epilogue"] == 0) & (c["phase"] == 0) & (c["polar"] == 0))
    implies(F["mel"] == 0, ~(fixed | packed | win) & (F["hoisted_passes"] == 0))
    # aligned block stores need the alignment; the store switches are honoured
    implies(F["aligned_stores"] == 1, (c["out_aligned_512"] == 1) & (c["spectrum"] == 1) & (c["dev_stores"] != 0))
    implies(F["nontemporal"] == 1, F["aligned_stores"] == 1)
    implies((F["nontemporal"] == 1) & (F["product"] == 1), c["dev_stores"] == 2)      # (the two dev forms exist with nt only)
    implies(F["persistent"] == 1, (F["nontemporal"] == 1) & (c["dev_persistent"] == 1))
    # every product form is somebody's choice; the dev forms need their switch, which a product build does not have
    assert sorted(set(f[F["product"] == 1])) == [i for i in range(len(names)) if m["product"][i]]
    implies(F["product"] == 0, c["dev_register_tables"] != 0)
    product_build = np.all([c[k] == v for k, v in PRODUCT.items()], axis=0)
    implies(product_build, F["product"] == 1)
    # ... and the headline calls get the headline forms there
    headline = product_build & bank_is["mel128"] & (c["hop"] == 256) & (c["contrast"] == 1) & (c["power2"] == 0) & \
        (c["channel_major"] == 0) & (c["phase"] == 0) & (c["polar"] == 0) & (c["epilogue"] == 0)
    implies(headline & (c["spectrum"] == 1), fixed & (F["aligned_stores"] == c["out_aligned_512"]))
    implies(headline & (c["spectrum"] == 0), fixed & (F["mel"] == 2))
