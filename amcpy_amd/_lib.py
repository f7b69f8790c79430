"""ctypes binding of libamcx.so (C ABI: include/amcx.h).

The HIP library is the product: if it cannot be loaded this module raises --
there is no CPU fallback anywhere in the package.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

_HERE = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get("AMCX_LIB", _HERE / "lib" / "libamcx.so"))

ABI_VERSION = 16        # the version this binding was written against; any library >= it will do (include/amcx.h)
ABI_MINOR = 2           # ... and, at that version, the additions it needs (AMCX_ABI_MINOR: 16.1 = training, 16.2 = the generator)
ABI_PATCH = 3           # ... and, at that minor, the additions it needs (AMCX_ABI_PATCH: 16.2.1 = the fading channel, 16.2.2 = continuous phase,
                        # 16.2.3 = carrier recovery)
NUM_FEATURES = 18
# feature masks (include/amcx.h, ABI 7): bit j - 1 = feature id j
FEATURES_ALL, FEATURES_NO_SPECTRAL, FEATURES_CUMULANTS = 0x3FFFF, 0x3FFFE, 0x3FE00
VARIANT_AUTO, VARIANT_BLOCK, VARIANT_WAVE = 0, 1, 2
VARIANTS = {"auto": VARIANT_AUTO, "block": VARIANT_BLOCK, "wave": VARIANT_WAVE}
OK, EINVAL, ENOTSUP, EHIP, ENODEV, ENOMEM, EIO = 0, -1, -2, -3, -4, -5, -6
SRC_C64, SRC_C128, SRC_F32_SPLIT, SRC_F64_SPLIT, SRC_SC16 = 0, 1, 2, 3, 4
SC16_SCALE = 2.0 ** -15                                 # the default sc16 scale: int16 onto [-1, 1) (ABI 9)
SRC_CI8, SRC_CU8 = 8, 9                                  # 8-bit IQ (ABI 10); 5, 6 and 7 are no kinds
IQ8_CI8, IQ8_CU8 = 0, 1                                  # AMCX_IQ8_*: the format argument of the 8-bit entries
IQ8_SCALE = 2.0 ** -7                                    # the default 8-bit scale: int8 onto [-1, 1)
ACT_RELU, ACT_TANH, ACT_SIGMOID = 0, 1, 2                # AMCX_ACT_* (ABI 8)
ACTIVATIONS = {"relu": ACT_RELU, "tanh": ACT_TANH, "sigmoid": ACT_SIGMOID}
ACT_NONE = 3                                             # AMCX_ACT_NONE (ABI 16): amcx_mlp_range_f32 only
OPT_RMSPROP, OPT_ADAM = 0, 1                             # AMCX_OPT_* (ABI 16.1)
SYNTH_RANDOM_PHASE, SYNTH_RANDOM_TIMING = 1, 2           # AMCX_SYNTH_* (ABI 16.2)
CHANNEL_RANDOM_PHASE = 1                                 # AMCX_CHANNEL_* (ABI 16.2.1)
CARRIER_GAIN, CARRIER_FREQ, CARRIER_PHASE, CARRIER_GIVEN = 1, 2, 4, 8      # AMCX_CARRIER_* (ABI 16.2.3)
# the carrier record (include/amcx.h, ABI 16.2.3), 32 bytes, as a numpy structured type
CARRIER_RECORD = [("phase_step", "<i8"), ("phase0", "<u4"), ("bin", "<i4"), ("frac", "<f4"), ("power", "<f4"), ("gain", "<f4"),
                  ("quality", "<f4")]
CHANNEL_MAX_PATHS, CHANNEL_MAX_SINUSOIDS, CHANNEL_MAX_DELAY = 16, 32, 1024


class UploadStats(C.Structure):
    """amcx_upload_stats (include/amcx.h)."""
    _fields_ = [("frames", C.c_int64), ("source_bytes", C.c_int64), ("pcie_bytes", C.c_int64),
                ("chunks", C.c_int32), ("threads", C.c_int32), ("plane_major", C.c_int32), ("from_file", C.c_int32),
                ("seconds", C.c_double), ("seconds_staging", C.c_double), ("seconds_waiting", C.c_double),
                ("seconds_prepare", C.c_double), ("seconds_tail", C.c_double)]


class Placement(C.Structure):
    """amcx_placement (include/amcx.h)."""
    _fields_ = [("device", C.c_int32), ("numa_node", C.c_int32), ("n_cpus", C.c_int32), ("n_cpus_allowed", C.c_int32),
                ("first_cpu", C.c_int32), ("last_cpu", C.c_int32), ("pci_bus_id", C.c_char * 32)]


# every symbol include/amcx.h declares: (restype, argtypes)
_i64, _i32, _vp, _fp = C.c_int64, C.c_int32, C.c_void_p, C.POINTER(C.c_float)
SIGNATURES = {
    "amcx_abi_version": (C.c_int, []),
    "amcx_strerror": (C.c_char_p, [C.c_int]),
    "amcx_last_hip_error": (C.c_char_p, []),
    "amcx_device_count": (C.c_int, []),
    "amcx_features18_c64": (C.c_int, [_vp, _i64, _i32, _i64, _vp, _i64, _vp]),
    "amcx_features18_c64_ex": (C.c_int, [_vp, _i64, _i32, _i64, _vp, _i64, _vp, _i32]),
    "amcx_features18_workspace_bytes": (_i64, [_i32, _i64, _i32]),
    "amcx_features18_c64_ws": (C.c_int, [_vp, _i64, _i32, _i64, _vp, _i64, _vp, _i32, _vp, _i64]),
    "amcx_features_c64_subset": (C.c_int, [_vp, _i64, _i32, _i64, _vp, _i64, _vp, _i32, C.c_uint32, _vp, _i64]),
    "amcx_kernel_name_subset": (C.c_int, [_i32, _i32, C.c_uint32, C.c_char_p, _i32]),
    "amcx_features_sc16_workspace_bytes": (_i64, [_i32, _i64, _i32]),
    "amcx_features_sc16": (C.c_int, [_vp, _i64, _i32, _i64, C.c_float, _vp, _i64, _vp, _i32, C.c_uint32, _vp, _i64]),
    "amcx_kernel_name_sc16": (C.c_int, [_i32, _i32, C.c_uint32, C.c_char_p, _i32]),
    "amcx_ctx_set_sc16_scale": (C.c_int, [_vp, C.c_float]),
    "amcx_ctx_features18_sc16_host": (C.c_int, [_vp, _vp, _i64, _i32, _i64, _vp, _i64, _i32]),
    "amcx_features_iq8_workspace_bytes": (_i64, [_i32, _i64, _i32]),
    "amcx_features_iq8": (C.c_int, [_vp, _i64, _i32, _i64, _i32, C.c_float, _vp, _i64, _vp, _i32, C.c_uint32, _vp, _i64]),
    "amcx_kernel_name_iq8": (C.c_int, [_i32, _i32, C.c_uint32, C.c_char_p, _i32]),
    "amcx_ctx_set_iq8_scale": (C.c_int, [_vp, C.c_float]),
    "amcx_ctx_features18_iq8_host": (C.c_int, [_vp, _vp, _i64, _i32, _i64, _i32, _vp, _i64, _i32]),
    "amcx_tune_decimate_out_samples": (_i64, [_i64, _i32, _i32]),
    "amcx_tune_decimate": (C.c_int, [_vp, _i32, _i64, C.c_float, C.c_uint64, C.c_uint64, _vp, _i32, _i32, _vp, _i64, _vp]),
    "amcx_tune_decimate_plan": (C.c_int, [_i32, _i32, C.POINTER(_i32), C.POINTER(_i32)]),
    "amcx_kernel_name_ddc": (C.c_int, [_i32, C.c_char_p, _i32]),
    "amcx_filter_bank_out_samples": (_i64, [_i64, _i32, _i32, _i32]),
    "amcx_filter_bank": (C.c_int, [_vp, _i32, _i64, C.c_float, C.c_uint64, C.c_uint64, C.c_uint64, _vp, _i32, _i32, _i32, _vp, _i64,
                                   _i64, _vp]),
    "amcx_filter_bank_plan": (C.c_int, [_i32, _i32, _i32, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32)]),
    "amcx_kernel_name_bank": (C.c_int, [_i32, C.c_char_p, _i32]),
    "amcx_resample_out_samples": (_i64, [_i64, _i32, _i32, _i32, _i32]),
    "amcx_resample": (C.c_int, [_vp, _i32, _i64, C.c_float, C.c_uint64, C.c_uint64, _vp, _i32, _i32, _i32, _i32, _vp, _i64, _vp]),
    "amcx_resample_plan": (C.c_int, [_i32, _i32, _i32, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32)]),
    "amcx_kernel_name_resample": (C.c_char_p, [_i32]),
    "amcx_row_power_c64": (C.c_int, [_vp, _i64, _i32, _i64, _vp, _vp]),
    "amcx_occupancy_workspace_bytes": (_i64, [_i32, _i64]),
    "amcx_occupancy_detect_f32": (C.c_int, [_vp, _i32, _i64, _i32, C.c_float, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "amcx_gather_rows_c64": (C.c_int, [_vp, _i64, _i32, _i64, _vp, _i64, _vp, _i64, _vp]),
    "amcx_kernel_name_occupancy": (C.c_char_p, [_i32]),
    "amcx_spectrogram_out_rows": (_i64, [_i64, _i32, _i32, _i32]),
    "amcx_spectrogram": (C.c_int, [_vp, _i32, _i64, C.c_float, _vp, _i32, _i32, _i32, _vp, _i64, _i64, _vp]),
    "amcx_spectrogram_plan": (C.c_int, [_i32, _i32, _i32, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32)]),
    "amcx_psd_detect_f32": (C.c_int, [_vp, _i64, _i32, _i64, _i32, C.c_float, _vp, _vp, _vp]),
    "amcx_kernel_name_psd": (C.c_int, [_i32, C.c_char_p, _i32]),
    "amcx_kernel_name_psd_detect": (C.c_char_p, []),
    "amcx_ctx_set_feature_mask": (C.c_int, [_vp, C.c_uint32]),
    "amcx_features18_c64_host": (C.c_int, [_vp, _i64, _i32, _i64, _vp, _i64, _i32, _i32]),
    "amcx_features18_c128_host": (C.c_int, [_vp, _i64, _i32, _i64, _vp, _i64, _i32, _i32]),
    "amcx_ctx_create": (C.c_int, [_i32, C.POINTER(_vp)]),
    "amcx_ctx_destroy": (C.c_int, [_vp]),
    "amcx_ctx_features18_c64_host": (C.c_int, [_vp, _vp, _i64, _i32, _i64, _vp, _i64, _i32]),
    "amcx_ctx_features18_c128_host": (C.c_int, [_vp, _vp, _i64, _i32, _i64, _vp, _i64, _i32]),
    "amcx_ctx_features18_strided_host": (C.c_int, [_vp, _vp, _vp, _i32, _i64, _i64, _i32, _i64, _i64, _i64,
                                                   _vp, _i64, _i32]),
    "amcx_stage_host": (C.c_int, [_vp, _vp, _i32, _i64, _i64, _i32, _i64, _i64, _i64, _i64, _i64, _vp, _i64, _i32,
                                  C.POINTER(_i32), C.POINTER(_i32)]),
    "amcx_ctx_features18_strided_file": (C.c_int, [_vp, _i32, _i64, _i64, _i32, _i64, _i64, _i32, _i64, _i64, _i64,
                                                   _vp, _i64, _i32]),
    "amcx_stage_file": (C.c_int, [_i32, _i64, _i64, _i32, _i64, _i64, _i32, _i64, _i64, _i64, _i64, _i64, _vp, _i64, _i32,
                                  C.POINTER(_i32), C.POINTER(_i32)]),
    "amcx_ctx_configure": (C.c_int, [_vp, _i32, _i64, _i32]),
    "amcx_ctx_upload_stats": (C.c_int, [_vp, C.POINTER(UploadStats)]),
    "amcx_pack_planes_c64": (C.c_int, [_vp, _i32, _i32, _i64, _i64, _i64, _i32, _vp, _i64, _i32, _vp]),
    "amcx_kernel_name": (C.c_int, [_i32, _i32, C.c_char_p, _i32]),
    "amcx_probe_read_bw": (C.c_int, [_vp, _i64, _vp, _vp]),
    "amcx_probe_fma_rate": (C.c_int, [C.c_double, _vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "amcx_device_pci_bus_id": (C.c_int, [_i32, C.c_char_p, _i32]),
    "amcx_numa_place": (C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(_i32), C.POINTER(_i32), _i32, C.POINTER(_i32)]),
    "amcx_ctx_bind_cpus": (C.c_int, [_vp, C.POINTER(_i32), _i32]),
    "amcx_ctx_placement": (C.c_int, [_vp, C.POINTER(Placement)]),
    "amcx_group_stats_f32": (C.c_int, [_vp, _i64, _i64, _i64, _i32, _vp, _vp, _vp]),
    "amcx_select_scale_f32": (C.c_int, [_vp, _i64, _i64, _vp, _i32, _vp, _vp, _vp, _i64, _vp]),
    "amcx_group_stats_workspace_bytes": (_i64, [_i64, _i64, _i32]),
    "amcx_group_stats_ws_f32": (C.c_int, [_vp, _i64, _i64, _i64, _i32, _vp, _vp, _vp, _i64, _vp]),
    "amcx_standardize_workspace_bytes": (_i64, [_i64, _i32]),
    "amcx_standardize_fit_transform_f32": (C.c_int, [_vp, _i64, _i64, _i32, C.POINTER(_i32), _i32, _vp, _i64,
                                                     _vp, _vp, _vp, _i64, _vp]),
    "amcx_mlp_params_floats": (_i64, [C.POINTER(_i32), _i32]),
    "amcx_mlp_classify_f32": (C.c_int, [_vp, _i64, _i64, _i32, C.POINTER(_i32), _i32, _vp, _vp, _vp, C.POINTER(_i32), _i32,
                                        _i32, _vp, _vp, _i64, _i64, _vp, _vp]),
    "amcx_mlp_kernel_name": (C.c_int, [C.POINTER(_i32), _i32, C.c_char_p, _i32]),
    "amcx_mlp_range_f32": (C.c_int, [_vp, _i64, _i64, _i32, C.POINTER(_i32), _i32, _vp, _vp, _vp, C.POINTER(_i32), _i32, _i32,
                                     _vp, _vp, _vp]),
    "amcx_mlp_q15_params_shorts": (_i64, [C.POINTER(_i32), _i32]),
    "amcx_mlp_classify_q15": (C.c_int, [_vp, _i64, _i64, _i32, C.POINTER(_i32), _i32, _vp, _vp, _vp, C.POINTER(_i32), _i32, _i32,
                                        _i32, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32), _vp, _vp, _i64, _i64, _vp, _vp, _vp]),
    "amcx_kernel_name_mlp_q15": (C.c_char_p, [_i32]),
    "amcx_mlp_train_state_floats": (_i64, [C.POINTER(_i32), _i32, C.c_uint32, _i32]),
    "amcx_mlp_train_workspace_floats": (_i64, [C.POINTER(_i32), _i32, _i32]),
    "amcx_mlp_train_f32": (C.c_int, [_vp, _i64, _i64, _i32, C.POINTER(_i32), _i32, _vp, _vp, _vp, _vp, _i64, _i64, C.POINTER(_i32), _i32,
                                     _i32, C.c_uint32, _i32, _i32, _i32, _vp, _vp, _vp, _fp, C.POINTER(C.c_uint32), _fp,
                                     C.POINTER(C.c_uint64), _i64, _i32, _vp, _vp]),
    "amcx_kernel_name_mlp_train": (C.c_char_p, [_i32, _i32]),
    "amcx_abi_minor": (C.c_int, []),
    "amcx_synth_plan": (C.c_int, [_i32, _i32, _i32, _i32, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32)]),
    "amcx_synth_c64": (C.c_int, [C.c_uint64, C.c_uint64, _i64, _i64, _i64, _i64, _vp, _i32, _vp, _i32, _i32, _i32, _i32, C.c_uint64,
                                 C.c_uint32, C.c_uint32, _vp, _i64, _vp, _vp]),
    "amcx_kernel_name_synth": (C.c_char_p, []),
    "amcx_abi_patch": (C.c_int, []),
    "amcx_channel_plan": (C.c_int, [_i32, _i32, _i32, _i32, C.POINTER(_i32), C.POINTER(_i32)]),
    "amcx_channel_c64": (C.c_int, [C.c_uint64, C.c_uint64, _i64, _i64, _i64, _vp, _i64, _vp, _i32, _i32, _i32, C.c_uint32, C.c_uint32,
                                   _vp, _i64, _vp, _i64, _vp]),
    "amcx_kernel_name_channel": (C.c_char_p, []),
    "amcx_synth_cpm_plan": (C.c_int, [_i32, _i32, _i32, _i64, _i64, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32)]),
    "amcx_synth_cpm_c64": (C.c_int, [C.c_uint64, C.c_uint64, _i64, _i64, _i64, _i64, _i32, _vp, _i32, C.c_uint32, _i32, _i32, _i32,
                                     C.c_uint64, C.c_uint32, C.c_uint32, _vp, _i64, _vp, _vp, _i32, _vp, _vp]),
    "amcx_kernel_name_synth_cpm": (C.c_char_p, []),
    "amcx_carrier_plan": (C.c_int, [_i32, C.POINTER(_i32), C.POINTER(_i32)]),
    "amcx_carrier_c64": (C.c_int, [_vp, _i64, _i32, _i64, _i32, _i32, C.c_uint32, _vp, _vp, _i64, _vp]),
    "amcx_kernel_name_carrier": (C.c_char_p, []),
}

_lib = None
_loaded_without_torch = False


class AmcxError(RuntimeError):
    def __init__(self, code: int, detail: str = ""):
        self.code = code
        super().__init__(f"amcx error {code}: {detail}")


def torch_wanted() -> bool:
    """False when the library was loaded on the system HIP runtime (``load(skip_torch=True)``, or AMCX_SKIP_TORCH=1 in
    the environment) and torch has not been imported: the host-buffer path (containers, files, calculate_features)
    needs neither torch nor its HIP runtime, and a process that never touches torch tensors -- the `extract`
    command line -- starts a second faster without the import."""
    import sys
    if "torch" in sys.modules:
        return True
    return not _loaded_without_torch and os.environ.get("AMCX_SKIP_TORCH", "0") != "1"


def load(skip_torch: bool = False) -> C.CDLL:
    """Load libamcx.so once.  torch (if installed) is imported first so that the
    library binds to the HIP runtime torch ships and device pointers are shared
    (unless the caller opts out -- ``skip_torch``, the command line's choice, or AMCX_SKIP_TORCH=1 -- see
    :func:`torch_wanted`: importing torch AFTER the library has loaded the system runtime would put two HIP
    runtimes into one process).  The opt-out is a property of this first call, not of the environment."""
    global _lib, _loaded_without_torch
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python amcpy_amd/csrc/build.py` "
            "(hipcc, gfx950). amcpy_amd has no CPU fallback.")
    import sys
    if "torch" in sys.modules or (not skip_torch and os.environ.get("AMCX_SKIP_TORCH", "0") != "1"):
        try:
            import torch  # noqa: F401  (side effect: loads torch's libamdhip64.so.7)
        except Exception:
            pass
    else:
        _loaded_without_torch = True
    lib = C.CDLL(str(LIB_PATH), mode=C.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is missing
        fn.restype, fn.argtypes = res, args
    got = lib.amcx_abi_version()
    if got < ABI_VERSION:
        raise ImportError(f"libamcx ABI {got} is older than the {ABI_VERSION} this binding needs")
    if got == ABI_VERSION and lib.amcx_abi_minor() < ABI_MINOR:
        raise ImportError(f"libamcx ABI {got}.{lib.amcx_abi_minor()} is older than the {ABI_VERSION}.{ABI_MINOR} this binding needs")
    if got == ABI_VERSION and lib.amcx_abi_minor() == ABI_MINOR and lib.amcx_abi_patch() < ABI_PATCH:
        raise ImportError(f"libamcx ABI {got}.{ABI_MINOR}.{lib.amcx_abi_patch()} is older than the {ABI_VERSION}.{ABI_MINOR}.{ABI_PATCH} this binding needs")
    _lib = lib
    return lib


def require_torch_runtime() -> None:
    """The tensor entry points hand torch's device pointers to the library: both must sit on ONE HIP runtime."""
    if _loaded_without_torch:
        raise RuntimeError("libamcx.so was loaded without torch (load(skip_torch=True) / AMCX_SKIP_TORCH=1: the system HIP "
                           "runtime); torch tensors belong to the runtime torch ships. Import torch before amcpy_amd loads "
                           "the library, or do not opt out.")


def check(code: int) -> None:
    if code == OK:
        return
    lib = load()
    msg = lib.amcx_strerror(code).decode()
    if code in (EHIP, EIO):
        msg += ": " + lib.amcx_last_hip_error().decode()
    if code == EIO:
        raise OSError(f"amcx: {msg}")
    if code == EINVAL:
        raise ValueError(f"amcx: {msg}")
    raise AmcxError(code, msg)


def kernel_name(frame_size: int, variant: int = VARIANT_AUTO) -> str:
    buf = C.create_string_buffer(128)
    check(load().amcx_kernel_name(frame_size, variant, buf, len(buf)))
    return buf.value.decode()


def feature_mask(feature_ids) -> int:
    """The mask of a set of feature ids (1 ... 18; repeats allowed).  KeyError for an unknown id, as the reference's
    calculate_features raises, before anything is launched; ValueError for an empty set."""
    import numbers
    mask = 0
    for fid in feature_ids:
        if isinstance(fid, bool) or not isinstance(fid, numbers.Integral) or not 1 <= int(fid) <= NUM_FEATURES:
            raise KeyError(fid)
        mask |= 1 << (int(fid) - 1)
    if mask == 0:
        raise ValueError("feature_ids is empty: at least one feature id (1 ... 18) is needed")
    return mask


def kernel_name_subset(frame_size: int, variant: int, mask: int) -> str:
    """amcx_kernel_name_subset: the kernel amcx_features_c64_subset runs for this mask (host-only)."""
    buf = C.create_string_buffer(128)
    check(load().amcx_kernel_name_subset(int(frame_size), int(variant), int(mask), buf, len(buf)))
    return buf.value.decode()


def kernel_name_sc16(frame_size: int, variant: int = VARIANT_AUTO, mask: int = FEATURES_ALL) -> str:
    """amcx_kernel_name_sc16: the kernel amcx_features_sc16 runs (host-only)."""
    buf = C.create_string_buffer(128)
    check(load().amcx_kernel_name_sc16(int(frame_size), int(variant), int(mask), buf, len(buf)))
    return buf.value.decode()


def kernel_name_iq8(frame_size: int, variant: int = VARIANT_AUTO, mask: int = FEATURES_ALL) -> str:
    """amcx_kernel_name_iq8: the feature kernel amcx_features_iq8 runs behind its widening kernel (host-only)."""
    buf = C.create_string_buffer(128)
    check(load().amcx_kernel_name_iq8(int(frame_size), int(variant), int(mask), buf, len(buf)))
    return buf.value.decode()


def kernel_name_ddc(src_kind: int) -> str:
    """amcx_kernel_name_ddc: the kernel amcx_tune_decimate runs for this source kind (host-only)."""
    buf = C.create_string_buffer(128)
    check(load().amcx_kernel_name_ddc(int(src_kind), buf, len(buf)))
    return buf.value.decode()


def tune_decimate_plan(n_taps: int, decim: int) -> tuple:
    """amcx_tune_decimate_plan -> (outputs per tile, most workgroups of the persistent grid) (host-only)."""
    tile, grid = C.c_int32(0), C.c_int32(0)
    check(load().amcx_tune_decimate_plan(int(n_taps), int(decim), C.byref(tile), C.byref(grid)))
    return tile.value, grid.value


def kernel_name_bank(src_kind: int) -> str:
    """amcx_kernel_name_bank: the kernel amcx_filter_bank runs for this source kind (host-only)."""
    buf = C.create_string_buffer(128)
    check(load().amcx_kernel_name_bank(int(src_kind), buf, len(buf)))
    return buf.value.decode()


def filter_bank_plan(n_taps: int, channels: int, decim: int) -> tuple:
    """amcx_filter_bank_plan -> (output instants per tile, most workgroups of the persistent grid, bytes of LDS) (host-only)."""
    tile, grid, lds = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    check(load().amcx_filter_bank_plan(int(n_taps), int(channels), int(decim), C.byref(tile), C.byref(grid), C.byref(lds)))
    return tile.value, grid.value, lds.value


def kernel_name_resample(src_kind: int) -> str:
    """amcx_kernel_name_resample: the kernel amcx_resample runs for this source kind (host-only)."""
    name = load().amcx_kernel_name_resample(int(src_kind))
    if name is None:
        raise ValueError(f"amcx: no resampler kernel for source kind {src_kind}")
    return name.decode()


def kernel_name_occupancy(which: int) -> str:
    """amcx_kernel_name_occupancy: 0 the row-power kernel, 1 the floor's, 2 the gather's, 3 ... 5 the count, scan and scatter
    launches (host-only)."""
    name = load().amcx_kernel_name_occupancy(int(which))
    if name is None:
        raise ValueError(f"amcx: no occupancy kernel number {which}")
    return name.decode()


def kernel_name_psd(src_kind: int) -> str:
    """amcx_kernel_name_psd: the kernel amcx_spectrogram runs for this source kind (host-only)."""
    buf = C.create_string_buffer(128)
    check(load().amcx_kernel_name_psd(int(src_kind), buf, len(buf)))
    return buf.value.decode()


def kernel_name_mlp_q15(which: int = 0) -> str:
    """amcx_kernel_name_mlp_q15: 0 the integer network's kernel, 1 the range kernel, 2 its initialising launch (host-only)."""
    name = load().amcx_kernel_name_mlp_q15(int(which))
    if name is None:
        raise ValueError(f"amcx: no fixed-point kernel number {which}")
    return name.decode()


def kernel_name_mlp_train(activation: str = "relu", optimizer: str = "rmsprop") -> str:
    """amcx_kernel_name_mlp_train: the training kernel of an (activation, optimizer) (host-only)."""
    name = load().amcx_kernel_name_mlp_train(ACTIVATIONS.get(activation, -2), {"rmsprop": OPT_RMSPROP, "adam": OPT_ADAM}.get(optimizer, -2))
    if name is None:
        raise ValueError(f"amcx: no training kernel for {activation!r} / {optimizer!r}")
    return name.decode()


def kernel_name_synth() -> str:
    """amcx_kernel_name_synth: the kernel amcx_synth_c64 runs (host-only)."""
    return load().amcx_kernel_name_synth().decode()


def kernel_name_channel() -> str:
    """amcx_kernel_name_channel: the kernel amcx_channel_c64 runs (host-only)."""
    return load().amcx_kernel_name_channel().decode()


def channel_plan(n_paths: int, n_sinusoids: int, interp_log2: int, max_delay: int) -> tuple:
    """amcx_channel_plan -> (outputs per tile, bytes of LDS) (host-only)."""
    tile, lds = C.c_int32(0), C.c_int32(0)
    check(load().amcx_channel_plan(int(n_paths), int(n_sinusoids), int(interp_log2), int(max_delay), C.byref(tile), C.byref(lds)))
    return tile.value, lds.value


def kernel_name_synth_cpm() -> str:
    """amcx_kernel_name_synth_cpm: the kernel amcx_synth_cpm_c64 runs (host-only)."""
    return load().amcx_kernel_name_synth_cpm().decode()


def synth_cpm_plan(n_taps: int, up: int, down: int, n_rows: int, row_samples: int) -> tuple:
    """amcx_synth_cpm_plan -> (samples per tile, bytes of LDS, segments a row is cut into) (host-only)."""
    tile, lds, seg = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    check(load().amcx_synth_cpm_plan(int(n_taps), int(up), int(down), int(n_rows), int(row_samples), C.byref(tile), C.byref(lds),
                                     C.byref(seg)))
    return tile.value, lds.value, seg.value


def kernel_name_carrier() -> str:
    """amcx_kernel_name_carrier: the kernel amcx_carrier_c64 runs (host-only)."""
    return load().amcx_kernel_name_carrier().decode()


def carrier_plan(n: int) -> tuple:
    """amcx_carrier_plan -> (rows a workgroup holds, bytes of static LDS) (host-only)."""
    rows, lds = C.c_int32(0), C.c_int32(0)
    check(load().amcx_carrier_plan(int(n), C.byref(rows), C.byref(lds)))
    return rows.value, lds.value


def synth_plan(order: int, n_taps: int, up: int, down: int) -> tuple:
    """amcx_synth_plan -> (samples per tile, bytes of LDS, most workgroups of the persistent grid) (host-only)."""
    tile, lds, grid = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    check(load().amcx_synth_plan(int(order), int(n_taps), int(up), int(down), C.byref(tile), C.byref(lds), C.byref(grid)))
    return tile.value, lds.value, grid.value


def kernel_name_psd_detect() -> str:
    """amcx_kernel_name_psd_detect: the kernel amcx_psd_detect_f32 runs (host-only)."""
    return load().amcx_kernel_name_psd_detect().decode()


def spectrogram_plan(nfft: int, hop: int, averages: int) -> tuple:
    """amcx_spectrogram_plan -> (segments per pass, bytes of LDS, most workgroups of the persistent grid) (host-only)."""
    segs, lds, grid = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    check(load().amcx_spectrogram_plan(int(nfft), int(hop), int(averages), C.byref(segs), C.byref(lds), C.byref(grid)))
    return segs.value, lds.value, grid.value


def resample_plan(n_taps: int, interp: int, decim: int) -> tuple:
    """amcx_resample_plan -> (outputs per tile, most samples a tile stages, most workgroups of the persistent grid, bytes of
    LDS) (host-only)."""
    tile, span, grid, lds = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
    check(load().amcx_resample_plan(int(n_taps), int(interp), int(decim), C.byref(tile), C.byref(span), C.byref(grid), C.byref(lds)))
    return tile.value, span.value, grid.value, lds.value


def numa_place(pci_bus_id: str, sysfs_root: str = "") -> tuple:
    """(node, [cpus]) local to the PCI device ``dddd:bb:dd.f`` according to ``<sysfs_root>/bus/pci/devices`` (default
    /sys): amcx_numa_place.  (-1, []) when the platform does not say.  Host-only: needs no GPU."""
    lib = load()
    node, n = C.c_int32(-1), C.c_int32(0)
    check(lib.amcx_numa_place(sysfs_root.encode(), pci_bus_id.encode(), C.byref(node), None, 0, C.byref(n)))
    cpus = (C.c_int32 * max(1, n.value))()
    check(lib.amcx_numa_place(sysfs_root.encode(), pci_bus_id.encode(), C.byref(node), cpus, n.value, C.byref(n)))
    return node.value, [int(c) for c in cpus[:n.value]]


def device_pci_bus_id(device: int) -> str:
    buf = C.create_string_buffer(32)
    check(load().amcx_device_pci_bus_id(int(device), buf, len(buf)))
    return buf.value.decode()


def probe_fma_rate(seconds: float = 1.0, stream: int = 0) -> dict:
    """amcx_probe_fma_rate on the current device: {"wave_instr_per_s", "clock_GHz"} (synchronises the stream)."""
    rate, clock = C.c_double(0.0), C.c_double(0.0)
    check(load().amcx_probe_fma_rate(float(seconds), stream or None, C.byref(rate), C.byref(clock)))
    return {"wave_instr_per_s": rate.value, "clock_GHz": clock.value}


class HostContext:
    """Reusable host-buffer context (amcx_ctx_*): a stream and growing device scratch kept
    across calls.  One per thread and device; freed with the object."""

    def __init__(self, device: int = 0):
        self._h = C.c_void_p()
        self.device = int(device)
        self.mask = FEATURES_ALL
        self.scales = {"sc16": SC16_SCALE, "iq8": IQ8_SCALE}       # what the library holds, per C setter
        check(load().amcx_ctx_create(self.device, C.byref(self._h)))

    def set_feature_mask(self, mask: int) -> None:
        """amcx_ctx_set_feature_mask: every later call computes only these features (NaN in the other columns)."""
        mask = int(mask)
        if mask != self.mask:
            check(load().amcx_ctx_set_feature_mask(self._h, mask))
            self.mask = mask

    def set_scale(self, fmt: str, scale: float) -> None:
        """amcx_ctx_set_sc16_scale / amcx_ctx_set_iq8_scale, whichever serves the format ``fmt``: what every later call on
        samples of that family multiplies a component by.  cf32 has none: nothing is set."""
        from . import _formats                             # (function-level: _formats reads this module's constants)
        family = _formats.get(fmt).family
        scale = C.c_float(scale).value
        if family is not None and scale != self.scales[family]:
            check(getattr(load(), f"amcx_ctx_set_{family}_scale")(self._h, scale))
            self.scales[family] = scale

    def run(self, x2, frame_size: int, out, variant: int) -> None:
        """x2: C-contiguous (F, L) complex64 / complex128 ndarray, or (F, L, 2) int16 (sc16) / int8 (ci8) / uint8 (cu8);
        out: (F, >=18) float32."""
        from . import _formats
        lib = load()
        fmt = _formats.by_plain(x2.dtype)
        if fmt is not None and fmt.family is not None:
            entry = getattr(lib, f"amcx_ctx_features18_{fmt.family}_host")
        else:
            entry = lib.amcx_ctx_features18_c128_host if x2.dtype == "complex128" else lib.amcx_ctx_features18_c64_host
        which = () if fmt is None or fmt.iq8 is None else (fmt.iq8,)          # the 8-bit entry alone is told which format
        check(entry(self._h, x2.ctypes.data, x2.shape[0], int(frame_size), x2.shape[1], *which,
                    out.ctypes.data, out.shape[1], int(variant)))

    def configure(self, threads: int = 0, slot_bytes: int = 0, round_on_device: int = -1) -> None:
        check(load().amcx_ctx_configure(self._h, int(threads), int(slot_bytes), int(round_on_device)))

    def run_strided(self, re_ptr: int, im_ptr, kind: int, n_snr: int, n_frames: int, frame_size: int,
                    strides, out, variant: int = VARIANT_AUTO) -> None:
        """amcx_ctx_features18_strided_host: `strides` = (snr, frame, sample) in source elements;
        out: C-contiguous (n_snr * n_frames, >= 18) float32.  The caller keeps the source alive."""
        check(load().amcx_ctx_features18_strided_host(
            self._h, re_ptr, im_ptr, int(kind), int(n_snr), int(n_frames), int(frame_size),
            int(strides[0]), int(strides[1]), int(strides[2]), out.ctypes.data, out.shape[1], int(variant)))

    def run_file(self, fd: int, re_offset: int, im_offset, kind: int, n_snr: int, n_frames: int, frame_size: int,
                 strides, out, variant: int = VARIANT_AUTO) -> None:
        """amcx_ctx_features18_strided_file: the container read from its file by the staging threads (byte
        offsets of the real / imaginary arrays; strides in elements).  OSError if a read fails."""
        check(load().amcx_ctx_features18_strided_file(
            self._h, int(fd), int(re_offset), -1 if im_offset is None else int(im_offset), int(kind), int(n_snr),
            int(n_frames), int(frame_size), int(strides[0]), int(strides[1]), int(strides[2]), out.ctypes.data,
            out.shape[1], int(variant)))

    def bind_cpus(self, cpus) -> None:
        """amcx_ctx_bind_cpus: the staging threads (and the caller during a large upload) on these CPUs; [] unbinds."""
        cpus = [int(c) for c in cpus]
        arr = (C.c_int32 * max(1, len(cpus)))(*cpus)
        check(load().amcx_ctx_bind_cpus(self._h, arr, len(cpus)))

    def placement(self) -> dict:
        pl = Placement()
        check(load().amcx_ctx_placement(self._h, C.byref(pl)))
        return {"device": pl.device, "numa_node": pl.numa_node, "n_cpus": pl.n_cpus, "n_cpus_allowed": pl.n_cpus_allowed,
                "first_cpu": pl.first_cpu, "last_cpu": pl.last_cpu, "pci_bus_id": pl.pci_bus_id.decode()}

    def upload_stats(self) -> dict:
        st = UploadStats()
        check(load().amcx_ctx_upload_stats(self._h, C.byref(st)))
        return {name: getattr(st, name) for name, _ in UploadStats._fields_}

    def close(self) -> None:
        if self._h:
            load().amcx_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
