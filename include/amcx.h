/*
 * amcx.h -- C ABI of the MI355X IQ feature-extraction engine (libamcx.so).
 *
 * The reference (ronnymilleo/amcpy) is pure Python and has no FFI layer; the
 * seams this ABI replaces are plain Python call sites:
 *
 *   per frame : amcpy.features.calculate_features(feature_ids, signal)
 *               src/amcpy/features.py:214-232   (18 feature fns :66-185)
 *   per batch : the `_Worker` loop body
 *               feature_matrix[snr, frame, :] = calculate_features(1..18, signal)
 *               src/amcpy/feature_extraction.py:30-39, fed by :64-72
 *
 * A binding is a ctypes stub of ~15 lines; see INTEGRATION.md.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++/torch types cross this boundary.
 *   - IQ layout: row-major frames of interleaved (re, im) float32 == numpy
 *     complex64 == the reference's (n_snr, n_frames, >=frame_size) container
 *     flattened to [n_frames][row_stride_elems] (README.md:60-73;
 *     feature_extraction.py:68 takes the first frame_size samples of a row).
 *   - output: out[f * out_row_stride + j], j = 0..17 is feature id j+1 of
 *     frame f, float32 (feature_extraction.py:35,56).  Caller allocates both
 *     buffers and keeps them alive until the stream has drained; the library
 *     holds no persistent state and never frees caller memory.
 *   - every function returns 0 or a negative AMCX_E* code and never throws.
 *     NaN/Inf in the data are not errors: a frame holding a non-finite sample
 *     yields 18 NaNs, as numpy's arithmetic does for the reference.
 *   - amplitude range: any normal float32 sample, at every frame size (the squares of samples
 *     below ~3e-19 underflow; a frame of nothing but non-negative reals that small is taken
 *     for zeros).  The block kernel stages each frame times an exact power of two and
 *     un-scales in fp64.  The throughput kernel's fp32 sums hold inside 1e-5 <~ rms|x| <~ 1e5;
 *     a frame outside that (or any of whose sums overflows: a single 1e7 sample among unit
 *     ones) is re-run on a copy multiplied by an exact power of two by the throughput kernel itself
 *     -- at the frame sizes 1024 ... 4096 right behind the batch it was found in (128, 256 and 512 take EVERY frame times a
 *     power of two, as the block kernel does: nothing to re-run), at 8192 in a pass of
 *     the quad at the end of the launch, at 16384 / 32768 at the end of every epoch of 2048 frames of a
 *     workgroup (a data set that is out of range throughout, e.g. raw 24-bit ADC counts, runs at half
 *     the normal rate) -- so
 *     results match the reference, which evaluates in complex128 (features.py:46-58), including
 *     the inf / 0 / denormals its float32 store produces (feature_extraction.py:35,56).
 *   - AMCX_VARIANT_WAVE / AUTO at a power-of-two frame size 128 ... 32768 is ONE launch on the stream; when
 *     it has completed every row is final (ABI 3 as built in rounds 2-3 took two launches and left out-of-range
 *     frames marked in band in between, and so did N = 8192 until late in round 4).  Frames with a phase step
 *     within an fp32 ulp of +-pi are finished exactly inside every throughput kernel.
 *   - PARITY CONTRACT with the reference (the executable form is tests/test_gpu_parity.py): features
 *     1-9 and 11 within 1e-5 relative of the reference's complex128 evaluation stored as float32;
 *     features 10, 12-18 (cumulants whose terms cancel) within 1e-5 of max(|value|, S), S the sum of
 *     the magnitudes of the terms of that cumulant's formula (the reference's own complex64 path is
 *     up to 8.5e-3 off in plain relative terms there).  EVERY frame, whatever the size of the sample: a
 *     frame one of whose cumulants cancels below what fp32 sums resolve (S < kappa x the first-order
 *     error scale of that cumulant, kappa = 4e-3 (2048 / N)^(1/3); ~0.7 % of the BASELINE configs' frames)
 *     is found by the kernel's finaliser and gets its moment sums from an fp64 sweep in the same launch
 *     (amcx_math.h: cancellation_suspect; until ABI 6's round-6 build samples of thousands of frames were
 *     held to a floored S with 0.1 % of the frames excepted).
 *   - DEVICE OWNERSHIP: the entry points that take device pointers launch on the calling thread's
 *     CURRENT HIP device.  The buffers and the stream must belong to it: on a multi-GPU node call
 *     hipSetDevice(d) (torch.cuda.set_device / `with torch.cuda.device(d)`) first.  A pointer
 *     that lives on another device is refused with AMCX_EINVAL (checked with
 *     hipPointerGetAttributes; a stream cannot be checked: passing another device's stream is a
 *     HIP launch error, AMCX_EHIP).  The host-buffer entries take a device index and switch to it
 *     themselves for the duration of the call.
 *   - re-entrant and thread-safe; launches are asynchronous on `hip_stream`
 *     (a hipStream_t, NULL = default stream); completion = caller's stream sync.
 *     The device entry points allocate nothing and never synchronise, so after one
 *     warm call per kernel and device they can be captured in a HIP graph.
 */
#ifndef AMCX_H_
#define AMCX_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version policy: the number goes up by one whenever entry points or constants are ADDED;
 * nothing that exists is ever removed or changes meaning under the same library name, so a binding
 * written against version v works with every library whose amcx_abi_version() >= v (and must
 * refuse an older one).  History: 1 = round 1-2 (features18, host / context entries, post kernels);
 * 2 = strided containers (amcx_ctx_features18_strided_host, amcx_stage_host, amcx_pack_planes_c64,
 * amcx_ctx_configure, amcx_ctx_upload_stats), device-ownership rule below made explicit;
 * 3 = single-read statistics with a caller workspace (amcx_group_stats_ws_f32,
 * amcx_group_stats_workspace_bytes), amcx_standardize_fit_transform_f32 / _workspace_bytes, and containers
 * read straight from their file (amcx_ctx_features18_strided_file, amcx_stage_file, AMCX_EIO);
 * 4 = host placement (amcx_numa_place, amcx_device_pci_bus_id, amcx_ctx_bind_cpus, amcx_ctx_placement: a context's
 * staging threads and pinned slots on the CPUs local to its device) and the instruction-issue ceiling probe
 * (amcx_probe_fma_rate);
 * 5 = frame sizes 16384 and 32768 (AMCX_MAX_FRAME_SIZE 32768, AMCX_MAX_BLOCK_FRAME_SIZE);
 * 6 = EVERY frame size 2 ... 32768: AMCX_MAX_BLOCK_FRAME_SIZE 32768 (8193 ... 32767 were AMCX_ENOTSUP but for 16384);
 * amcx_features18_c64_ws / amcx_features18_workspace_bytes;
 * 7 = feature subsets: AMCX_FEATURES_*, amcx_features_c64_subset, amcx_ctx_set_feature_mask, amcx_kernel_name_subset;
 * 8 = classification on the device: AMCX_ACT_*, amcx_mlp_params_floats, amcx_mlp_classify_f32, amcx_mlp_kernel_name;
 * 9 = frames of 16-bit integer IQ (sc16): amcx_features_sc16, amcx_features_sc16_workspace_bytes, amcx_kernel_name_sc16,
 * AMCX_SRC_SC16 for the strided host / file entries and amcx_stage_host / _file, amcx_ctx_set_sc16_scale,
 * amcx_ctx_features18_sc16_host;
 * 10 = frames of 8-bit IQ (ci8, cu8), widened on the device: AMCX_IQ8_*, amcx_features_iq8, amcx_features_iq8_workspace_bytes,
 * amcx_kernel_name_iq8, AMCX_SRC_CI8 / AMCX_SRC_CU8 for the strided host / file entries and amcx_stage_host / _file,
 * amcx_ctx_set_iq8_scale, amcx_ctx_features18_iq8_host;
 * 11 = the digital down-converter; 12 = the polyphase filter bank; 13 = the rational resampler; 14 = occupancy detection
 * (all listed behind the define); 15 = the Welch spectrogram and its per-row detection; 16 = fixed-point deployment of the
 * classifier's network (range calibration and 16-bit integer inference).
 * AMCX_ABI_MINOR counts what has been ADDED since the version last changed -- new entries and constants, nothing existing changed:
 * 16.1 = training of the classifier's network, one workgroup per model; 16.2 = the waveform generator.
 * AMCX_ABI_PATCH counts in the same way what has been added since the minor last changed: 16.2.1 = the fading multipath channel;
 * 16.2.2 = the generator's continuous-phase modulations; 16.2.3 = blind carrier recovery. */
#define AMCX_ABI_VERSION 16
#define AMCX_ABI_MINOR 2
#define AMCX_ABI_PATCH 3
/* The define, version by version, the newest first (a binding may look for the line of the version it was written against):
 *   ABI 16.2.3: AMCX_ABI_PATCH 3          -- blind carrier recovery: AMCX_CARRIER_*, amcx_carrier_c64, amcx_carrier_plan,
 *                                            amcx_kernel_name_carrier
 *   ABI 16.2.2: AMCX_ABI_PATCH 2          -- continuous-phase modulations (FSK, MSK, GMSK): amcx_synth_cpm_c64,
 *                                            amcx_synth_cpm_plan, amcx_kernel_name_synth_cpm
 *   ABI 16.2.1: AMCX_ABI_PATCH 1          -- the fading channel: AMCX_CHANNEL_*, amcx_channel_c64, amcx_channel_plan,
 *                                            amcx_kernel_name_channel, amcx_abi_patch
 *   ABI 16.2: AMCX_ABI_MINOR 2            -- the waveform generator: AMCX_SYNTH_*, amcx_synth_c64, amcx_synth_plan,
 *                                            amcx_kernel_name_synth
 *   ABI 16.1: AMCX_ABI_MINOR 1            -- training: AMCX_OPT_*, amcx_mlp_train_f32, amcx_mlp_train_state_floats,
 *                                            amcx_mlp_train_workspace_floats, amcx_kernel_name_mlp_train, amcx_abi_minor
 *   ABI 16: the line above               -- fixed-point deployment: AMCX_ACT_NONE, amcx_mlp_range_f32, amcx_mlp_classify_q15,
 *                                            amcx_mlp_q15_params_shorts, amcx_kernel_name_mlp_q15
 *   ABI 15: #define AMCX_ABI_VERSION 15   -- the spectrogram: amcx_spectrogram, amcx_spectrogram_out_rows, amcx_spectrogram_plan,
 *                                            amcx_psd_detect_f32, amcx_kernel_name_psd, amcx_kernel_name_psd_detect
 *   ABI 14: #define AMCX_ABI_VERSION 14   -- occupancy detection: amcx_row_power_c64, amcx_occupancy_workspace_bytes,
 *                                            amcx_occupancy_detect_f32, amcx_gather_rows_c64, amcx_kernel_name_occupancy
 *   ABI 13: #define AMCX_ABI_VERSION 13   -- the rational resampler: amcx_resample, amcx_resample_out_samples,
 *                                            amcx_resample_plan, amcx_kernel_name_resample
 *   ABI 12: #define AMCX_ABI_VERSION 12   -- the polyphase filter bank: amcx_filter_bank, amcx_filter_bank_out_samples,
 *                                            amcx_filter_bank_plan, amcx_kernel_name_bank
 *   ABI 11: #define AMCX_ABI_VERSION 11   -- the digital down-converter: amcx_tune_decimate, amcx_tune_decimate_out_samples,
 *                                            amcx_tune_decimate_plan, amcx_kernel_name_ddc
 *   ABI 10: #define AMCX_ABI_VERSION 10   -- 8-bit IQ (ci8, cu8), widened on the device */
#define AMCX_NUM_FEATURES 18

/* FEATURE MASKS (ABI 7): bit j - 1 stands for feature id j (1 gamma_max ... 18 |C63|).  The reference's default selection,
 * FeatureConfig.used = (2, 4, 6, 8, 12, 14) read as 0-based columns, is sum(1 << c) = 0x5154 (ids 3, 5, 7, 9, 13, 15). */
#define AMCX_FEATURES_ALL 0x3FFFF
#define AMCX_FEATURES_NO_SPECTRAL 0x3FFFE  /* f2 ... f18: everything but gamma_max, the only feature that needs the FFT */
#define AMCX_FEATURES_CUMULANTS 0x3FE00    /* f10 ... f18: the moment sums alone (no FFT, no angle, no envelope) */

/* error codes */
#define AMCX_OK 0
#define AMCX_EINVAL (-1)   /* null pointer, negative count, bad stride, frame_size out of range */
#define AMCX_ENOTSUP (-2)  /* requested kernel variant cannot handle this frame_size */
#define AMCX_EHIP (-3)     /* HIP runtime / launch failure (see amcx_last_hip_error) */
#define AMCX_ENODEV (-4)   /* no usable gfx950 device */
#define AMCX_ENOMEM (-5)   /* device allocation failed (host-buffer entry point only) */
#define AMCX_EIO (-6)      /* a read from the container's file failed or the file ends inside the variable
                              (the *_file entries; amcx_last_hip_error() holds the errno text) */

/* kernel variants (amcx_features18_c64_ex) */
#define AMCX_VARIANT_AUTO 0     /* fastest kernel that supports frame_size */
#define AMCX_VARIANT_BLOCK 1    /* one 256-thread workgroup per frame, frame staged in LDS,
                                   radix-2 LDS FFT (power of two), Bluestein chirp-z FFT (every
                                   other N >= 65: both spectra in LDS up to 4096; 4097..8191 a
                                   16384-point convolution with the chirp's spectrum held in
                                   registers) or direct O(N^2) fp64 DFT (N <= 64); fp64
                                   accumulation.  Above 8192 samples (ABI 6) one 1024-thread
                                   workgroup per frame, the frame read where it lies, the phase in
                                   LDS, the spectral peak by a chirp-z / plain FFT run in place on a
                                   global workspace (amcx_features18_c64_ws below) or, without one,
                                   as the DFT by its definition with exact twiddle indices, O(N^2);
                                   2 <= frame_size <= AMCX_MAX_BLOCK_FRAME_SIZE */
#define AMCX_VARIANT_WAVE 2     /* the throughput kernels: the frame held in registers, register
                                   FFT with LDS exchanges, fp32 sums with an fp64 finaliser, frames
                                   outside the fp32 range re-run inside the launch; frame_size a
                                   power of two, 128 ... 32768 (1024 ... 4096: one wavefront per
                                   frame; 128 ... 512: four frames per wavefront; 8192: four waves
                                   per frame, 16384 / 32768: eight / sixteen) */

#define AMCX_MIN_FRAME_SIZE 2
#define AMCX_MAX_FRAME_SIZE 32768       /* the reference takes any frame_size (config.py:96; np.fft.fft, features.py:68); this
                                           library: every size 2 ... 32768 (ABI 6; ABI 5: 2 ... 8192 and the powers of two
                                           16384, 32768).  Larger: AMCX_EINVAL. */
#define AMCX_MAX_BLOCK_FRAME_SIZE 32768 /* AMCX_VARIANT_BLOCK (and with it every size that is not a power of two) ends here */

int amcx_abi_version(void);
const char* amcx_strerror(int code);
/* text of the last HIP error seen by the calling thread ("" if none) */
const char* amcx_last_hip_error(void);
/* number of visible devices whose architecture is gfx950; <0 on error */
int amcx_device_count(void);

/*
 * All 18 features of n_frames frames, device buffers.
 * Replaces the `_Worker.run` loop body, feature_extraction.py:30-39, for a
 * whole (n_snr * n_frames) block at once.
 *   iq_dev            device pointer, complex64 [n_frames][row_stride_elems]
 *   row_stride_elems  distance between frame starts in complex elements, >= frame_size
 *   out_dev           device pointer, float32 [n_frames][out_row_stride]
 *   out_row_stride    in floats, >= 18
 *   hip_stream        hipStream_t or NULL
 * n_frames == 0 is a valid no-op.
 */
int amcx_features18_c64(const void* iq_dev, int64_t n_frames, int32_t frame_size,
                        int64_t row_stride_elems, float* out_dev, int64_t out_row_stride,
                        void* hip_stream);

/* Same, with an explicit kernel variant (tests and benchmarks). */
int amcx_features18_c64_ex(const void* iq_dev, int64_t n_frames, int32_t frame_size,
                           int64_t row_stride_elems, float* out_dev, int64_t out_row_stride,
                           void* hip_stream, int32_t variant);

/*
 * ABI 6.  The any-size path above 8192 samples (AMCX_VARIANT_BLOCK there; AUTO where frame_size is not a power of
 * two) has two forms of its spectral term: an FFT through a device workspace -- Bluestein's chirp-z as a 32768- /
 * 65536-point circular convolution run in place on one private buffer per workgroup, the plain transform at 16384 /
 * 32768 -- and, without one, the DFT by its definition (O(N^2), ~100x slower at 32767; same results within the parity
 * contract).  amcx_features18_c64 / _ex take the workspace from the stream-ordered allocator (hipMallocAsync /
 * hipFreeAsync on hip_stream), except while the stream is being captured into a graph or when the allocator fails:
 * then they run the form that needs none (AMCX_VERBOSE=1 in the environment: one line on stderr, once per process,
 * when that happens -- the kernel's name and the results do not show which form ran; a caller whose device memory is
 * owned by another allocator, e.g. torch's caching one, should hand in the workspace itself).
 * amcx_features18_c64_ws takes the caller's: at least
 * amcx_features18_workspace_bytes(frame_size, n_frames, variant) bytes of device memory (contents undefined before,
 * garbage after; 8-byte aligned; on the current device) for the full number of frames in flight, fewer bytes mean fewer
 * workgroups, less than one workgroup's share (or NULL) the workspace-free form.  _workspace_bytes is 0 for every
 * frame size and variant that needs none (all of 2 ... 8192, and the WAVE kernels), -1 for arguments the call itself
 * would refuse.  Every other frame size: _ws behaves exactly as _ex and ignores the workspace.
 */
int64_t amcx_features18_workspace_bytes(int32_t frame_size, int64_t n_frames, int32_t variant);
int amcx_features18_c64_ws(const void* iq_dev, int64_t n_frames, int32_t frame_size,
                           int64_t row_stride_elems, float* out_dev, int64_t out_row_stride,
                           void* hip_stream, int32_t variant, void* workspace_dev, int64_t workspace_bytes);

/*
 * ABI 7.  Only the features in feature_mask (FEATURE MASKS above), same rules and arguments as amcx_features18_c64_ws
 * (workspace_dev may be NULL).  The output stays 18 wide: a column in the mask holds the feature BIT-IDENTICAL to what
 * amcx_features18_c64_ws writes for the same frame, frame size and variant; a column outside it holds NaN.  A mask of 0, or
 * one with a bit at or above bit 18, is AMCX_EINVAL before any HIP call.  The kernel is chosen by the mask:
 *   bit 0 set (gamma_max asked for)              the 18-feature kernel;
 *   mask within AMCX_FEATURES_CUMULANTS          the CUMULANTS plan: a streaming reduction of the 15 moment sums;
 *   otherwise                                    the NO-SPECTRAL plan: the 18-feature kernel without its FFT.
 * The plans exist for AMCX_VARIANT_WAVE / AUTO at 128 ... 4096 (amcx_kernel_name_subset names them).  Every other frame
 * size, and AMCX_VARIANT_BLOCK, runs the 18-feature kernel and then a pass that writes NaN outside the mask: correct, no
 * faster.
 */
int amcx_features_c64_subset(const void* iq_dev, int64_t n_frames, int32_t frame_size, int64_t row_stride_elems,
                             float* out_dev, int64_t out_row_stride, void* hip_stream, int32_t variant, uint32_t feature_mask,
                             void* workspace_dev, int64_t workspace_bytes);

/*
 * ABI 9.  Frames of 16-bit integer IQ (UHD sc16, SigMF ci16_le), read as they lie: half the bytes of complex64.
 *   - A sample is two little-endian int16, I then Q, interleaved (numpy int16 of shape (..., L, 2)); row_stride_samples
 *     counts samples of 4 bytes, any value >= frame_size; only the first frame_size samples of a row are read.  iq_dev
 *     must be 4-byte aligned.
 *   - The frame's value is complex64((float)I * scale, (float)Q * scale): int16 -> float32 is exact, and the product is
 *     ONE float32 multiplication per component, nothing fused into it.  scale is a finite float32 > 0 (2^-15 maps the
 *     int16 range onto [-1, 1)); NaN, infinite, 0 or negative is AMCX_EINVAL, checked beside the other arguments, before
 *     a device is looked for.
 *   - The features are those amcx_features_c64_subset writes for the SAME variant and feature_mask on that complex64
 *     frame, BIT FOR BIT: the NaN / inf / 0 pattern, the range re-run, the +-pi-tie path, the fp64 cancellation path and
 *     the NaN of the columns not asked for included.  Every slow path re-reads the frame through the same loader and the
 *     same multiplication.
 *   - AMCX_VARIANT_WAVE / AUTO at 128 ... 4096 run kernels that read sc16 themselves (amcx_kernel_name_sc16 names them:
 *     "...sc16..."), and need no workspace.  Every other frame size, and AMCX_VARIANT_BLOCK, widens the frames into the
 *     head of the workspace (8 * frame_size * n_frames bytes rounded up to 256; workspace_dev must then be 8-byte aligned:
 *     the copy is complex64 -- otherwise AMCX_EINVAL) and runs the complex64 path on the copy,
 *     handing it the rest of the workspace under the rules of amcx_features18_c64_ws.
 *     amcx_features_sc16_workspace_bytes is 0 where a kernel reads sc16 itself, otherwise the widened copy plus
 *     amcx_features18_workspace_bytes (-1 for arguments amcx_features_sc16 refuses); a workspace smaller than the widened
 *     copy, where one is needed, is AMCX_EINVAL.
 * Asynchronous on the caller's stream, allocates nothing, and can be captured into a graph wherever
 * amcx_features_c64_subset can.
 */
int64_t amcx_features_sc16_workspace_bytes(int32_t frame_size, int64_t n_frames, int32_t variant);
int amcx_features_sc16(const void* iq_dev, int64_t n_frames, int32_t frame_size, int64_t row_stride_samples, float scale,
                       float* out_dev, int64_t out_row_stride, void* hip_stream, int32_t variant, uint32_t feature_mask,
                       void* workspace_dev, int64_t workspace_bytes);

/*
 * ABI 10.  Frames of 8-bit IQ, what the cheap receivers write (cu8: the RTL-SDR family; ci8: HackRF- and Airspy-class tools,
 * SigMF ci8 / cu8): a quarter of the bytes of complex64.  No feature kernel reads 8-bit samples: the device widens the
 * frames first, with one small kernel, and runs the kernels that exist.
 *   - A sample is two bytes, I then Q.  AMCX_IQ8_CI8: the bytes are int8.  AMCX_IQ8_CU8: the bytes are uint8 around the zero
 *     level 128, a component is (int8)(byte ^ 0x80), i.e. byte - 128.  (The other convention for cu8, a zero level of 127.5,
 *     is not offered: it has no integer form, and a caller who wants it subtracts 0.5 * scale from the mean himself.)  Any
 *     other format is AMCX_EINVAL.  row_stride_samples counts samples of 2 bytes, any value >= frame_size; only the first
 *     frame_size samples of a row are read.  iq_dev must be 2-byte aligned.
 *   - The frame's value is complex64((float)i * scale, (float)q * scale), i and q in -128 ... 127: ONE float32 multiplication
 *     per component.  scale follows amcx_features_sc16's rules (finite float32 > 0, otherwise AMCX_EINVAL, checked before a
 *     device is looked for); 2^-7 maps the range onto [-1, 1).
 *   - The widening to int16 is sign extension, so the features are amcx_features_sc16's on (int16)x with the same scale,
 *     variant and feature_mask BIT FOR BIT, and thereby amcx_features_c64_subset's on the widened complex64 frame, every
 *     slow path and the NaN of the columns not asked for included.
 *   - A workspace is ALWAYS needed (for n_frames > 0), 8-byte aligned: its head takes the widened copy -- sc16,
 *     4 * frame_size * n_frames bytes rounded up to 256, where amcx_features_sc16 runs an sc16 kernel (128 ... 4096 with
 *     AMCX_VARIANT_WAVE / AUTO); complex64, 8 * frame_size * n_frames rounded up to 256, everywhere else -- and the rest is
 *     handed on as amcx_features_sc16 hands it on.  amcx_features_iq8_workspace_bytes says how much: the head, plus
 *     amcx_features18_workspace_bytes where the copy is complex64; 0 for n_frames == 0, -1 for arguments amcx_features_iq8
 *     refuses.  No workspace, one smaller than the head, or one that is not 8-byte aligned is AMCX_EINVAL.  A caller whose
 *     8-bit data outlives one call and who wants the resident rate keeps the widened sc16 instead (README).
 * Asynchronous on the caller's stream, allocates nothing, and can be captured into a graph wherever amcx_features_sc16 can.
 */
#define AMCX_IQ8_CI8 0
#define AMCX_IQ8_CU8 1
int64_t amcx_features_iq8_workspace_bytes(int32_t frame_size, int64_t n_frames, int32_t variant);
int amcx_features_iq8(const void* iq_dev, int64_t n_frames, int32_t frame_size, int64_t row_stride_samples, int32_t format,
                      float scale, float* out_dev, int64_t out_row_stride, void* hip_stream, int32_t variant,
                      uint32_t feature_mask, void* workspace_dev, int64_t workspace_bytes);

/*
 * ABI 11.  THE DIGITAL DOWN-CONVERTER: tune, low-pass and decimate a recording where it lies.  A receiver records a band several
 * times wider than the emitter, which sits off centre; the features want it at 0 Hz and filling its band.
 *   - src_dev is ONE contiguous stream of n_samples samples, src_kind AMCX_SRC_C64, AMCX_SRC_SC16, AMCX_SRC_CI8 or AMCX_SRC_CU8
 *     (defined below; every other kind is AMCX_EINVAL).  A sample's value x[n] is what ABI 9 / 10 define: for the integer
 *     kinds complex64((float)i * scale, (float)q * scale), cu8 as byte - 128; scale is ignored for complex64.
 *   - taps_dev: n_taps REAL float32 taps h[0 .. n_taps - 1] in device memory; decim: the decimation factor D.  With T = n_taps:
 *         phi(n) = (phase0 + n * phase_step) mod 2^64        (uint64 arithmetic, exact; n counts THIS CALL's input samples)
 *         v[n]   = x[n] * exp(+2 pi j * phi(n) / 2^64)
 *         y[m]   = sum_{k = 0 .. T-1} h[k] * v[m D + T - 1 - k],   m = 0 ... M - 1,   M = n_samples < T ? 0 : (n_samples - T) / D + 1
 *     i.e. numpy.convolve(v, h, "valid")[::D]; y is packed complex64 at out_c64_dev, which has room for out_capacity_samples.
 *     To move a signal at +f Hz to 0: phase_step = round(-f / fs * 2^64) mod 2^64.  A caller that continues a stream passes
 *     phase0 + consumed * phase_step.  The angle is formed from the top 32 bits of phi (1.5e-9 rad, far below an fp32 sine's
 *     rounding); range reduction is integer and exact.
 *   - limits: 1 <= n_taps <= 2048, 1 <= decim <= 4096 (decim > n_taps is legal: samples are skipped), 0 <= n_samples < 2^40.
 *     Alignment: src 8 / 4 / 2 bytes (c64 / sc16 / 8-bit), taps 4, out 8.
 *   - POSITION INDEPENDENCE: the bits of y[m] depend only on its T input samples, the taps and phi at those samples -- not on m's
 *     place in the call, on n_samples, on the grid or on which load read the samples; each output is summed in one fixed order
 *     of k.  A stream cut into calls at any multiple of D, with phase0 advanced, gives the one-call result bit for bit.
 *   - phi = 0 IS EXACT: the mixer value is exactly 1 + 0j there (for every phi < 2^32).  With phase0 = phase_step = 0, T = 1,
 *     h = {1}, D = 1 the output is the widened input bit for bit.
 *   - accuracy: |y[m] - exact| <= (T + 8) 2^-24 sum_k |h[k]| |x[m D + T - 1 - k]| (tests/test_gpu_ddc.py).
 * Asynchronous on the caller's stream, allocates nothing, capturable in a graph.  The checks come before any device call, in
 * this order: src_kind; scale (integer kinds only: finite float32 > 0); n_taps, decim and n_samples ranges; out_capacity_samples
 * >= M; M == 0 is AMCX_OK here, null pointers allowed; null pointers and alignment; a pointer on another device.
 * amcx_tune_decimate_out_samples: M, or -1 for arguments the entry refuses.
 * amcx_tune_decimate_plan (host-only): how a call is cut -- *tile_outputs consecutive outputs per tile (a tile's input span,
 * (tile - 1) D + T samples, is staged in LDS), a persistent grid of at most *max_workgroups workgroups on the current device
 * (256 CUs assumed where there is none); either pointer may be NULL.  AMCX_EINVAL for n_taps / decim out of range.
 */
int64_t amcx_tune_decimate_out_samples(int64_t n_samples, int32_t n_taps, int32_t decim);
int amcx_tune_decimate(const void* src_dev, int32_t src_kind, int64_t n_samples, float scale, uint64_t phase0,
                       uint64_t phase_step, const float* taps_dev, int32_t n_taps, int32_t decim, void* out_c64_dev,
                       int64_t out_capacity_samples, void* hip_stream);
int amcx_tune_decimate_plan(int32_t n_taps, int32_t decim, int32_t* tile_outputs, int32_t* max_workgroups);

/*
 * ABI 12.  THE POLYPHASE FILTER BANK: every channel of a raster from ONE pass over a recording.  A wideband recording holds many
 * emitters on a channel raster; C calls of amcx_tune_decimate read it C times and spend T / D FMAs per input sample each.
 * The bank reads it once: 2 P FMAs per input sample and one C-point transform per output instant.
 *   - src_dev, src_kind, n_samples, scale, phase0, phase_step, taps_dev: as amcx_tune_decimate (the same sample values, the same
 *     mixer).  C = channels, a power of two 2 ... 256; T = n_taps, 1 ... 4096; P = ceil(T / C) taps per branch (a tap index >= T
 *     does not exist: it is never read, and no sample is read for it); D = decim, 1 ... C, any integer (D = C: critically
 *     sampled, D = C / 2: 2x oversampled); 0 <= n_samples < 2^40; sample_index0: the absolute index of src[0] in the stream.
 *         phi(n)  = (phase0 + n * phase_step) mod 2^64                  (n counts THIS CALL's samples)
 *         v[n]    = x[n] * exp(+2 pi j * phi(n) / 2^64)                  (phi < 2^32: v = x, the product is skipped)
 *         a(n)    = (sample_index0 + n) mod C
 *         n_m     = m D + T - 1,   M = n_samples < T ? 0 : (n_samples - T) / D + 1
 *         y[c,m]  = sum_{k < T} h[k] * v[n_m - k] * exp(-2 pi j * c * a(n_m - k) / C)      c = 0 ... C - 1, m = 0 ... M - 1
 *         out[c * out_channel_stride + m] = y[c,m]                       (packed complex64, CHANNEL-MAJOR, stride >= M)
 *     Channel c is centred at +c / C cycles per sample of the pre-mixed stream -- FFT order: c > C / 2 are negative
 *     frequencies; the pre-mixer offsets the whole raster.  By definition channel c is amcx_tune_decimate with
 *     phase_step_c = phase_step - c 2^64 / C and phase0_c = phase0 - c (sample_index0 mod C) 2^64 / C, both mod 2^64.
 *   - computed as branch sums u_m[p] = sum_{q < P, p + q C < T} h[p + q C] v[n_m - p - q C] (one product, then one FMA per
 *     component in ascending q), and y[., m] = the unnormalised C-point DFT with kernel e^{+2 pi j c r / C} of
 *     g[r] = u_m[(r + a(n_m)) mod C]; radix 2, twiddles exact at +-1 and +-j (amcx_bank_kernel.h).
 *   - POSITION INDEPENDENCE: the bits of y[c,m] depend only on the T samples, the taps, phi at those samples and a(n_m) -- not on
 *     m's place in the call, the tile, the grid, the lane or which load read a sample.  A stream cut into calls at any multiple
 *     of D, with phase0 and sample_index0 advanced, gives the one-call result bit for bit.
 *   - the four formats give the same bits as the complex64 call on the widened samples.
 *   - EXACT CASE: phase0 = phase_step = 0, T = 1, h = {1}, D = 1, C = 2 or 4: y[c,n] is x[n] times an exact power of j.
 *   - accuracy: |y - exact| <= (P + 8 + 7 log2 C) 2^-24 sum_k |h[k]| |x[n_m - k]| (tests/bank_ref.py).
 * Asynchronous on the caller's stream, allocates nothing, capturable in a graph.  out_capacity_samples is the capacity of the
 * whole buffer: (C - 1) * out_channel_stride + M must fit.  The checks come before any device call, in this order: src_kind;
 * scale (integer kinds only); channels (a power of two in range), n_taps, decim and n_samples ranges; out_channel_stride >= M,
 * and the capacity; M == 0 is AMCX_OK here, null pointers allowed; null pointers and alignment (src 8 / 4 / 2, taps 4, out 8);
 * a pointer on another device.
 * amcx_filter_bank_out_samples: M, or -1 for arguments the entry refuses.
 * amcx_filter_bank_plan (host-only): *tile_outputs consecutive output instants per tile, a persistent grid of at most
 * *max_workgroups workgroups on the current device (256 CUs assumed where there is none), *lds_bytes of dynamic LDS per
 * workgroup; any pointer may be NULL.  AMCX_EINVAL for channels / n_taps / decim out of range.
 */
int64_t amcx_filter_bank_out_samples(int64_t n_samples, int32_t n_taps, int32_t channels, int32_t decim);
int amcx_filter_bank(const void* src_dev, int32_t src_kind, int64_t n_samples, float scale, uint64_t phase0,
                     uint64_t phase_step, uint64_t sample_index0, const float* taps_dev, int32_t n_taps,
                     int32_t channels, int32_t decim, void* out_c64_dev, int64_t out_channel_stride,
                     int64_t out_capacity_samples, void* hip_stream);
int amcx_filter_bank_plan(int32_t n_taps, int32_t channels, int32_t decim, int32_t* tile_outputs,
                          int32_t* max_workgroups, int32_t* lds_bytes);

/*
 * ABI 13.  THE RATIONAL RESAMPLER: tune, low-pass and change the sample rate by L / D where a recording lies.  The down-converter
 * changes the rate by an integer only; an emitter whose band is fs / 3.9 wide then comes out anywhere between r and 2 r times
 * oversampled, and the features (the spectral peak, the cumulants) change with that ratio.
 *   - src_dev, src_kind, n_samples, scale, phase0, phase_step, taps_dev: as amcx_tune_decimate (the same sample values, the same
 *     mixer).  T = n_taps REAL taps h[0 .. T - 1] given AT THE UPSAMPLED RATE (L times the input's); L = interp, D = decim;
 *     tau0 = phase_index0, the phase of the first output, 0 <= tau0 < L.  Conceptually v is zero-stuffed by L, filtered with h,
 *     and every D-th result is kept; nothing is zero-stuffed in practice:
 *         phi(n) = (phase0 + n * phase_step) mod 2^64        (uint64 arithmetic, exact; n counts THIS CALL's input samples)
 *         v[n]   = x[n] * exp(+2 pi j * phi(n) / 2^64)        (phi < 2^32: v = x, the product is skipped)
 *         P      = ceil(T / L)                                taps of the longest phase
 *         t_m    = m D + tau0,   p_m = t_m mod L,   n_m = (P - 1) + floor(t_m / L)
 *         y[m]   = sum_{q >= 0, p_m + q L < T} h[p_m + q L] * v[n_m - q],   m = 0 ... M - 1
 *         M      = S < P ? 0 : ((S - P + 1) L - 1 - tau0 < 0 ? 0 : ((S - P + 1) L - 1 - tau0) / D + 1),   S = n_samples
 *     y is packed complex64 at out_c64_dev, which has room for out_capacity_samples.
 *   - limits: 1 <= n_taps <= 4096, 1 <= interp <= 256, 1 <= decim <= 4096, 0 <= n_samples < 2^40, 0 <= phase_index0 < interp.
 *     Alignment: src 8 / 4 / 2 bytes (c64 / sc16 / 8-bit), taps 4, out 8.
 *   - EMPTY PHASES: a phase with no tap (T < L, p_m >= T) gives exactly +0 + 0j.  A tap index >= T does not exist: it is never
 *     read, and no sample enters a sum for it.  (A tile's span of samples is loaded whole -- the oldest sample of a phase one
 *     tap short, the samples between two windows where D > P L: all inside [0, n_samples), mixed, and never multiplied into
 *     an output, so a NaN there reaches nothing.)
 *   - GAIN: none is applied; the taps carry it (a low-pass with DC gain L keeps the signal's amplitude).
 *   - SUMMATION ORDER: one product h[p_m] v[n_m], then one FMA per component in ascending q.  With L = 1 (tau0 = 0) that is the
 *     order k = 0 ... T - 1 of amcx_tune_decimate: for n_taps <= 2048 the output equals amcx_tune_decimate's bit for bit, in all
 *     four formats.
 *   - POSITION INDEPENDENCE: the bits of y[m] depend only on its samples, the taps, phi at those samples and p_m -- not on m's
 *     place in the call, the tile, the grid, the lane or which load read a sample.
 *   - CONTINUATION: a stream cut after any whole number M of outputs equals one call bit for bit: the next call drops
 *     floor((M D + tau0) / L) inputs, takes phase_index0 = (M D + tau0) mod L and phase0 advanced by the dropped inputs.
 *   - the four formats give the same bits as the complex64 call on the widened samples.
 *   - accuracy: |y[m] - exact| <= (P + 8) 2^-24 sum_q |h[p_m + q L]| |x[n_m - q]| (tests/resample_ref.py).
 * Asynchronous on the caller's stream, allocates nothing, capturable in a graph.  The checks come before any device call, in
 * this order: src_kind; scale (integer kinds only: finite float32 > 0); n_taps, interp, decim, n_samples and phase_index0 ranges;
 * out_capacity_samples >= M; M == 0 is AMCX_OK here, null pointers allowed; null pointers and alignment; a pointer on another
 * device.
 * amcx_resample_out_samples: M, or -1 for arguments the entry refuses.
 * amcx_resample_plan (host-only): how a call is cut -- *tile_outputs consecutive outputs per tile, no tile's input span (staged
 * in LDS) longer than *max_span_samples, a persistent grid of at most *max_workgroups workgroups on the current device (256 CUs
 * assumed where there is none), *lds_bytes of dynamic LDS per workgroup (the padded span and the phase-major taps); any pointer
 * may be NULL.  AMCX_EINVAL for n_taps / interp / decim out of range.
 */
int64_t amcx_resample_out_samples(int64_t n_samples, int32_t n_taps, int32_t interp, int32_t decim, int32_t phase_index0);
int amcx_resample(const void* src_dev, int32_t src_kind, int64_t n_samples, float scale, uint64_t phase0, uint64_t phase_step,
                  const float* taps_dev, int32_t n_taps, int32_t interp, int32_t decim, int32_t phase_index0,
                  void* out_c64_dev, int64_t out_capacity_samples, void* hip_stream);
int amcx_resample_plan(int32_t n_taps, int32_t interp, int32_t decim, int32_t* tile_outputs, int32_t* max_span_samples,
                       int32_t* max_workgroups, int32_t* lds_bytes);

/*
 * OCCUPANCY DETECTION on a (channel x frame) grid (ABI 14; amcpy_amd/csrc/amcx_occupancy_kernels.h).  A CELL is one frame of
 * N complex64 samples of one channel: row r = c K + k of the (C K, N) matrix the filter bank's output is cut into.  All three
 * entries are asynchronous on the caller's stream, allocate nothing and are capturable in a graph; their checks come before
 * any device call, in the order each states.  Global memory is written with ordinary vector stores; no workgroup waits for
 * another; no atomics.
 *
 * amcx_row_power_c64: power_dev[r] = sum_{n < N} re^2 + im^2 in float32, r < n_rows, N = row_samples, row r at rows_dev +
 * r * row_stride_samples samples.
 *   - THE ORDER depends on N alone (the kernel header states it: one accumulator per lane, s = fma(im, im, fma(re, re, s)) over
 *     the lane's sample pairs in ascending order, then a fixed 6-level tree over the 64 lanes).
 *   - POSITION INDEPENDENCE: a row's bits depend on its N samples alone -- not on its place in the call, the stride, whether the
 *     row begins on 16 bytes (16-byte loads) or only on 8 (8-byte loads of the same samples), the grid or the batch.
 *   - accuracy: every term is non-negative, so |p - exact| <= B 2^-24 exact with B = 4 ceil(N / 128) + 8 (tests/occupancy_ref.py).
 *     NaN and Inf propagate as IEEE 754 says.  Nothing outside a row's N samples is read.
 *   - checks: n_rows >= 0 and 2 <= row_samples <= AMCX_MAX_FRAME_SIZE; row_stride_samples >= row_samples (and n_rows times it
 *     below 2^58); n_rows == 0 is AMCX_OK here, null pointers allowed; null pointers and alignment (rows 8, power 4); a pointer
 *     on another device.
 *
 * amcx_occupancy_detect_f32: per frame k, across the C = channels values power_dev[c K + k] (K = n_frames, packed):
 *     floor_dev[k]       = the element of rank floor_rank (0-based, ascending, NaN last) of those C values
 *     mask_dev[c K + k]  = power_dev[c K + k] > threshold * floor_dev[k] ? 1 : 0     (ONE float32 product, one IEEE comparison:
 *                          a NaN power, or a NaN floor, is not occupied)
 *     rows_dev[0 .. n)   = the occupied rows r = c K + k in ASCENDING order, *count_dev = n; entries at and beyond n are not
 *                          written.  rows_dev has room for C K entries.
 *   Every result is exactly what numpy float32 gives (tests/occupancy_ref.py, numpy_detect).  mask_dev and rows_dev may each
 *   be NULL (not wanted); count_dev is required with rows_dev and may be given without it.  With rows_dev or count_dev the
 *   entry needs workspace_dev of at least amcx_occupancy_workspace_bytes bytes (block counts; it is overwritten).  Launches:
 *   the floor; the mask and the counts of blocks of 256 rows; ONE workgroup that scans the counts; the scatter.
 *   - limits: 2 <= channels <= 256 (any integer), n_frames >= 0, channels * n_frames < 2^31, 0 <= floor_rank < channels,
 *     threshold a finite float32 > 0.
 *   - checks: those limits; workspace_bytes (where rows_dev or count_dev is given); n_frames == 0 is AMCX_OK here, null
 *     pointers allowed, nothing written; null pointers (power, floor; count with rows; the workspace) and alignment (4 bytes
 *     each); a pointer on another device.
 * amcx_occupancy_workspace_bytes: the bytes that call needs, monotone in both arguments; -1 for a grid the entry refuses.
 *
 * amcx_gather_rows_c64: dst_dev[i * dst_stride_samples + n] = src_dev[index_dev[i] * row_stride_samples + n], i < n_index,
 * n < row_samples -- a copy, bit for bit, with 16-byte accesses where both rows begin on 16 bytes and 8-byte otherwise.  An
 * index outside [0, n_src_rows) gives a row of NaN + NaN j, and nothing outside the source's rows is read.  The feature
 * kernels take a constant row stride: this copy is what lets them run on the occupied cells alone.
 *   - checks: n_src_rows >= 0, n_index >= 0, 2 <= row_samples <= AMCX_MAX_FRAME_SIZE; both strides >= row_samples; n_index == 0
 *     is AMCX_OK here, null pointers allowed; null pointers (src only where n_src_rows > 0) and alignment (src 8, index 4,
 *     dst 8); a pointer on another device.
 */
int amcx_row_power_c64(const void* rows_dev, int64_t n_rows, int32_t row_samples, int64_t row_stride_samples,
                       float* power_dev, void* hip_stream);
int64_t amcx_occupancy_workspace_bytes(int32_t channels, int64_t n_frames);            /* -1 for refused arguments */
int amcx_occupancy_detect_f32(const float* power_dev, int32_t channels, int64_t n_frames, int32_t floor_rank,
                              float threshold, float* floor_dev, uint8_t* mask_dev, int32_t* rows_dev,
                              int32_t* count_dev, void* workspace_dev, int64_t workspace_bytes, void* hip_stream);
int amcx_gather_rows_c64(const void* src_dev, int64_t n_src_rows, int32_t row_samples, int64_t row_stride_samples,
                         const int32_t* index_dev, int64_t n_index, void* dst_dev, int64_t dst_stride_samples,
                         void* hip_stream);

/*
 * ABI 15.  THE WELCH SPECTROGRAM of a raw stream, and the detection of occupied bins per row (amcpy_amd/csrc/amcx_psd_kernel.h):
 * where the emitters of an unknown band are, with no channel raster.  Both entries are asynchronous on the caller's stream,
 * allocate nothing and are capturable in a graph; their checks come before any device call, in the order each states.
 *
 * amcx_spectrogram: S = n_samples samples at src_dev (src_kind, scale: as amcx_tune_decimate), window_dev[0 .. nfft) float32,
 * segment s begins at sample s * hop, A = averages:
 *     xw_s[n]       = window[n] * x[s hop + n]                               one float32 product per component
 *     X_s[b]        = sum_{n < nfft} xw_s[n] exp(-2 pi j b n / nfft)          b = 0 ... nfft - 1, FFT order (b > nfft / 2:
 *                                                                            negative frequencies)
 *     psd[r, b]     = sum_{a < A} |X_{r A + a}[b]|^2                          at psd_dev + r * row_stride + b, float32
 *     nseg = S >= nfft ? floor((S - nfft) / hop) + 1 : 0,   R = floor(nseg / A)   (amcx_spectrogram_out_rows; a partial last
 *                                                                            row is dropped, never a partial sum)
 *   The rows 0 ... n_rows - 1 are written, n_rows <= R.  No normalisation: 1 / (A sum window^2) is the caller's.
 *   - ONE OPERATION SEQUENCE PER nfft (the kernel header writes it down; tests/psd_ref.py restates it in numpy float32): radix-2
 *     decimation in frequency, log2 nfft stages; twiddles are the down-converter's mixer at exact integer angles (1 and -j are
 *     exact); products as the filter bank forms them, (fma(a, c, -(b d)), fma(a, d, b c)); EVERY butterfly multiplies, also
 *     by 1; |X|^2 = fma(im, im, re re); the row sum is ((p_0 + p_1) + p_2) + ... in ascending a.  It depends on nfft alone.
 *   - POSITION INDEPENDENCE: a row's bits depend on its (A - 1) hop + nfft samples and the window, on nothing else: not on
 *     whether the span begins on 16 bytes (any sample-aligned src_dev: 8, 4 or 2 bytes), the row's index, row_stride or
 *     n_rows.  A stream cut into calls after any whole number of rows equals one call bit for bit.
 *   - FORMATS: the rows of an sc16 / ci8 / cu8 stream are the bits of the complex64 call on the widened samples.
 *   - Nothing outside [src, src + S) and [window, window + nfft) is read; nothing but the n_rows rows' nfft columns is written.
 *   - accuracy: |psd - exact| <= the bound tests/psd_ref.py derives from the sequence, of the form
 *     (6 log2 nfft + 1) 2^-24 sum_n |xw[n]| per transform output, carried through the squares and the row sum.
 *   - limits: nfft a power of two 64 ... 4096; 1 <= hop <= 65536 (a hop above nfft leaves gaps, which are never read);
 *     1 <= averages <= 65536; 0 <= n_samples < 2^40.
 *   - checks: src_kind and, for the integer kinds, scale (finite, > 0); those limits, 0 <= n_rows <= R, row_stride >= nfft (and
 *     n_rows times it at most 2^58); n_rows == 0 is AMCX_OK here, null pointers allowed; null pointers and alignment (src: a
 *     sample; window 4, psd 4); a pointer on another device.
 * amcx_spectrogram_out_rows: R, or -1 for arguments the entry refuses.  amcx_spectrogram_plan (host-only): the segments a
 * workgroup transforms at a time (of that many DIFFERENT rows), the bytes of LDS, the most workgroups of the persistent grid.
 *
 * amcx_psd_detect_f32: per row r of psd_dev (n_rows rows of `bins` float32 at row_stride):
 *     floor_dev[r]          = the element of rank floor_rank (0-based, ascending, NaN last) of the row's bins values
 *     mask_dev[r bins + b]  = psd[r, b] > threshold * floor_dev[r] ? 1 : 0     (ONE float32 product, one IEEE comparison: a NaN
 *                             is not occupied); packed rows of `bins` bytes; mask_dev may be NULL (not wanted)
 *   Exactly what numpy float32 gives: amcx_occupancy_detect_f32's definitions, transposed, without the row list.
 *   - checks: n_rows >= 0, 2 <= bins <= 4096 (any integer), 0 <= floor_rank < bins, threshold a finite float32 > 0;
 *     row_stride >= bins (and n_rows times it at most 2^58); n_rows == 0 is AMCX_OK here, null pointers allowed; null pointers
 *     (psd, floor) and alignment (4 bytes each); a pointer on another device.
 */
int64_t amcx_spectrogram_out_rows(int64_t n_samples, int32_t nfft, int32_t hop, int32_t averages);        /* -1 for refused arguments */
int amcx_spectrogram(const void* src_dev, int32_t src_kind, int64_t n_samples, float scale, const float* window_dev,
                     int32_t nfft, int32_t hop, int32_t averages, float* psd_dev, int64_t row_stride, int64_t n_rows,
                     void* hip_stream);
int amcx_spectrogram_plan(int32_t nfft, int32_t hop, int32_t averages, int32_t* segments_per_pass, int32_t* lds_bytes,
                          int32_t* max_workgroups);
int amcx_psd_detect_f32(const float* psd_dev, int64_t n_rows, int32_t bins, int64_t row_stride, int32_t floor_rank,
                        float threshold, float* floor_dev, uint8_t* mask_dev, void* hip_stream);

/*
 * Same computation for HOST buffers (numpy arrays): allocates device scratch,
 * copies in, runs the kernel on `device`, copies the (n_frames x 18) result
 * back and returns when it is in `out_host`.  Replaces a direct
 * calculate_features(...) call, features.py:214-232, without torch.
 * This is NOT a CPU implementation: it fails with AMCX_ENODEV without a GPU.
 */
int amcx_features18_c64_host(const void* iq_host, int64_t n_frames, int32_t frame_size,
                             int64_t row_stride_elems, float* out_host, int64_t out_row_stride,
                             int32_t device, int32_t variant);

/*
 * Same for a HOST container of complex128 (MATLAB doubles, what scipy.io.loadmat
 * returns for the reference's all_modulations.mat, feature_extraction.py:46-48):
 * rows are rounded to complex64 (round-to-nearest-even, identical to numpy's astype and
 * to the GPU's conversion) by the staging copy into pinned memory that has to happen
 * anyway, so PCIe carries 8 B/sample (amcx_ctx_configure(..., round_on_device = 1) sends
 * the doubles and rounds on the GPU instead).  row_stride_elems is in complex128 elements.
 */
int amcx_features18_c128_host(const void* iq_host, int64_t n_frames, int32_t frame_size,
                              int64_t row_stride_elems, float* out_host, int64_t out_row_stride,
                              int32_t device, int32_t variant);

/*
 * The same two host-buffer entry points over a reusable context: the context owns a
 * HIP stream and device scratch that only grows, so calling per frame in a loop -- the
 * reference's own usage pattern, calculate_features once per queue item
 * (feature_extraction.py:30-39) -- costs two small copies and the launches instead of
 * hipMalloc / hipFree / stream creation per call.  Small row-major calls (one chunk, under
 * 1 MiB) are replayed as a HIP GRAPH: copy in, conversion, kernels and copy out are captured
 * once per shape (frames, frame size, variant, element type; four shapes cached) and a call
 * is one hipGraphLaunch and one synchronisation (39 us per 2048-sample frame against 47 us as
 * separate runtime calls); AMCX_NO_GRAPH=1 in the environment turns that off.  A context belongs to one device and
 * must not be used by two threads at once (one context per thread).  amcx_ctx_destroy
 * accepts NULL.  The one-shot entry points above are these with a context that lives
 * for the duration of the call.
 */
typedef struct amcx_ctx amcx_ctx;
int amcx_ctx_create(int32_t device, amcx_ctx** ctx_out);
int amcx_ctx_destroy(amcx_ctx* ctx);
int amcx_ctx_features18_c64_host(amcx_ctx* ctx, const void* iq_host, int64_t n_frames,
                                 int32_t frame_size, int64_t row_stride_elems, float* out_host,
                                 int64_t out_row_stride, int32_t variant);
int amcx_ctx_features18_c128_host(amcx_ctx* ctx, const void* iq_host, int64_t n_frames,
                                  int32_t frame_size, int64_t row_stride_elems, float* out_host,
                                  int64_t out_row_stride, int32_t variant);
/* ABI 9: rows of sc16 (amcx_features_sc16: int16 I, int16 Q; row_stride_samples in samples of 4 bytes) in host memory.
 * They go over the link as they lie, 4 bytes per sample, and are never widened on the host; the device runs what
 * amcx_features_sc16 runs, with the context's scale (amcx_ctx_set_sc16_scale) and feature mask. */
int amcx_ctx_features18_sc16_host(amcx_ctx* ctx, const void* iq_host, int64_t n_frames,
                                  int32_t frame_size, int64_t row_stride_samples, float* out_host,
                                  int64_t out_row_stride, int32_t variant);
/* ABI 9: what every later sc16 call of this context multiplies an int16 component by (default 2^-15).  AMCX_EINVAL for a
 * scale that is NaN, infinite, 0 or negative, or while a call is running on the context. */
int amcx_ctx_set_sc16_scale(amcx_ctx* ctx, float scale);
/* ABI 10: rows of 8-bit IQ (amcx_features_iq8: format AMCX_IQ8_CI8 / AMCX_IQ8_CU8, row_stride_samples in samples of 2 bytes)
 * in host memory.  They go over the link as they lie, 2 bytes per sample; the device widens them and runs what
 * amcx_features_iq8 runs, with the context's 8-bit scale (amcx_ctx_set_iq8_scale) and feature mask. */
int amcx_ctx_features18_iq8_host(amcx_ctx* ctx, const void* iq_host, int64_t n_frames, int32_t frame_size,
                                 int64_t row_stride_samples, int32_t format, float* out_host, int64_t out_row_stride,
                                 int32_t variant);
/* ABI 10: what every later 8-bit call of this context multiplies a component by (default 2^-7); rules as
 * amcx_ctx_set_sc16_scale. */
int amcx_ctx_set_iq8_scale(amcx_ctx* ctx, float scale);

/*
 * Name of the kernel `variant` resolves to for this frame_size (as it shows in
 * rocprofv3 kernel traces), written NUL-terminated into buf.  Returns 0, or
 * AMCX_ENOTSUP / AMCX_EINVAL.
 */
int amcx_kernel_name(int32_t frame_size, int32_t variant, char* buf, int32_t buf_len);

/* ABI 7: the same for amcx_features_c64_subset with this feature_mask (host-only, no GPU needed): a plan kernel
 * (amcx_features_subset_wave_kernel<N, P> / amcx_features_subset_short_kernel<N, P>, P = 1 no-spectral, 2 cumulants), or
 * the 18-feature kernel amcx_kernel_name names (followed by amcx_mask_columns_kernel unless the mask is
 * AMCX_FEATURES_ALL).  AMCX_EINVAL for an invalid mask. */
int amcx_kernel_name_subset(int32_t frame_size, int32_t variant, uint32_t feature_mask, char* buf, int32_t buf_len);
/* ABI 9: the same for amcx_features_sc16 -- an sc16 kernel at 128 ... 4096 (WAVE / AUTO), otherwise the complex64 kernel
 * that runs on the widened copy. */
int amcx_kernel_name_sc16(int32_t frame_size, int32_t variant, uint32_t feature_mask, char* buf, int32_t buf_len);
/* ABI 10: the same for amcx_features_iq8, the FEATURE kernel that runs behind amcx_iq8_to_sc16_kernel /
 * amcx_iq8_to_c64_kernel: amcx_kernel_name_sc16's answer. */
int amcx_kernel_name_iq8(int32_t frame_size, int32_t variant, uint32_t feature_mask, char* buf, int32_t buf_len);
/* ABI 11: the kernel amcx_tune_decimate runs for this src_kind (host-only): amcx_ddc_c64_kernel, amcx_ddc_sc16_kernel, or
 * amcx_ddc_iq8_kernel for both 8-bit kinds.  AMCX_EINVAL for another kind. */
int amcx_kernel_name_ddc(int32_t src_kind, char* buf, int32_t buf_len);
/* ABI 12: the kernel amcx_filter_bank runs for this src_kind (host-only): amcx_bank_c64_kernel, amcx_bank_sc16_kernel, or
 * amcx_bank_iq8_kernel for both 8-bit kinds; AMCX_EINVAL for any other kind. */
int amcx_kernel_name_bank(int32_t src_kind, char* buf, int32_t buf_len);
/* ABI 13: the kernel amcx_resample runs for this src_kind (host-only), a static string: amcx_resample_c64_kernel,
 * amcx_resample_sc16_kernel, or amcx_resample_iq8_kernel for both 8-bit kinds; NULL for any other kind. */
const char* amcx_kernel_name_resample(int32_t src_kind);

/* ABI 14: the kernels of occupancy detection (host-only), static strings: 0 amcx_row_power_kernel, 1 amcx_occupancy_detect_kernel
 * (the floor), 2 amcx_gather_rows_kernel, and the three launches behind the floor: 3 amcx_occupancy_count_kernel,
 * 4 amcx_occupancy_scan_kernel, 5 amcx_occupancy_scatter_kernel; NULL for any other number. */
const char* amcx_kernel_name_occupancy(int32_t which);   /* 0 power, 1 detect, 2 gather */
/* ABI 15: the kernel amcx_spectrogram runs for this src_kind (host-only): amcx_spectrogram_c64_kernel, amcx_spectrogram_sc16_kernel
 * or, for ci8 and cu8, amcx_spectrogram_iq8_kernel; AMCX_EINVAL for another kind.  And amcx_psd_detect_f32's, a static string. */
int amcx_kernel_name_psd(int32_t src_kind, char* buf, int32_t buf_len);
const char* amcx_kernel_name_psd_detect(void);

/* ABI 7: every later host-buffer call of this context (amcx_ctx_features18_c64_host / _c128_host / _strided_host /
 * _strided_file) computes only the features in feature_mask, as amcx_features_c64_subset does (AMCX_FEATURES_ALL: the
 * default, the 18-feature path).  AMCX_EINVAL for an invalid mask or while a call is running on the context. */
int amcx_ctx_set_feature_mask(amcx_ctx* ctx, uint32_t feature_mask);

/*
 * The real-data path: all 18 features of every frame of a HOST container indexed
 * [snr][frame][sample] with ARBITRARY element strides -- what the reference slices frame by frame
 * out of the array scipy.io.loadmat returned (feature_extraction.py:46-48,64-72: Fortran-ordered,
 * complex128, rows longer than frame_size).  Frame g = snr * n_frames + frame, the order the
 * reference enqueues them in; out_host[g * out_row_stride + j] = feature j + 1.
 *
 *   kind      AMCX_SRC_C64 / AMCX_SRC_C128: `re` points at interleaved (re, im) float32 / float64,
 *             `im` is ignored.  AMCX_SRC_F32_SPLIT / AMCX_SRC_F64_SPLIT: `re` and `im` are two
 *             separate real arrays with the same strides (how a MATLAB v5 file stores a complex
 *             variable; im == NULL: a real signal).  Doubles are rounded to float32 to nearest even
 *             (== numpy astype), by the staging threads on their way to pinned memory.
 *             AMCX_SRC_SC16 (ABI 9): `re` points at interleaved (I, Q) int16, an element is one sample of 4 bytes,
 *             `im` is ignored; the value of a sample is amcx_features_sc16's with the context's scale
 *             (amcx_ctx_set_sc16_scale).  Staged and uploaded as it lies (upload_stats.pcie_bytes = 4 bytes per
 *             sample).  Row layouts only (stride_sample == 1): a plane-major layout is AMCX_ENOTSUP.
 *             AMCX_SRC_CI8 / AMCX_SRC_CU8 (ABI 10): `re` points at interleaved (I, Q) bytes, an element is one sample of 2
 *             bytes, `im` is ignored; the value of a sample is amcx_features_iq8's with the context's 8-bit scale
 *             (amcx_ctx_set_iq8_scale).  Staged and uploaded as it lies (upload_stats.pcie_bytes = 2 bytes per sample),
 *             widened by the device.  Row layouts only, as sc16.  Kinds 5, 6 and 7 are no kinds: AMCX_EINVAL.
 *   strides   in ELEMENTS of the source (complex elements for the interleaved kinds), all >= 0.
 *             One of them must be 1:
 *               stride_sample == 1 (C order)        rows go up in chunks of whole frames and the
 *                                                   kernel runs on chunk k while chunk k+1 uploads;
 *               stride_snr == 1 or stride_frame == 1 (Fortran order, as loadmat returns it)
 *                                                   contiguous sample planes go up as they lie and
 *                                                   a device kernel transposes them to frame-major
 *                                                   (amcx_pack_planes_c64); the feature kernel runs
 *                                                   once, after the last plane.
 *             Otherwise AMCX_ENOTSUP (make a contiguous copy first).
 *
 * Pageable memory is fine (that is the point): a pool of host threads copies runs into three pinned
 * slots while the copy engine drains them -- ~55 GB/s of PCIe, i.e. ~110 GB/s of complex128 source.
 * Blocks until out_host is complete.  One context per thread.
 */
#define AMCX_SRC_C64 0
#define AMCX_SRC_C128 1
#define AMCX_SRC_F32_SPLIT 2
#define AMCX_SRC_F64_SPLIT 3
#define AMCX_SRC_SC16 4
#define AMCX_SRC_CI8 8      /* (5, 6 and 7 stay AMCX_EINVAL) */
#define AMCX_SRC_CU8 9
int amcx_ctx_features18_strided_host(amcx_ctx* ctx, const void* re, const void* im, int32_t kind,
                                     int64_t n_snr, int64_t n_frames, int32_t frame_size,
                                     int64_t stride_snr, int64_t stride_frame, int64_t stride_sample,
                                     float* out_host, int64_t out_row_stride, int32_t variant);

/*
 * The host half on its own (no device involved; works without a GPU): stage `n_units` units of the
 * container, starting at `first_unit`, into `dst` as packed complex64, with `threads` host threads.
 * A unit is a frame (row-major containers: dst[unit][sample]) or a sample plane (plane-major:
 * dst[unit][position], position order as amcx_pack_planes_c64's inner_snr says); *plane_major and
 * *inner_snr report which (either may be NULL).  For callers that run their own copy engine -- and
 * how the staging and rounding logic is tested where there is no GPU.  AMCX_SRC_SC16: rows only, staged as packed sc16
 * (4 bytes per sample, dst_bytes accordingly); AMCX_SRC_CI8 / _CU8 likewise, 2 bytes per sample.
 */
int amcx_stage_host(const void* re, const void* im, int32_t kind, int64_t n_snr, int64_t n_frames,
                    int32_t frame_size, int64_t stride_snr, int64_t stride_frame, int64_t stride_sample,
                    int64_t first_unit, int64_t n_units, void* dst, int64_t dst_bytes, int32_t threads,
                    int32_t* plane_major, int32_t* inner_snr);

/*
 * The same two entries for a container that is still in its FILE: fd is an open descriptor (the library
 * neither closes nor seeks it: every read is a pread), re_offset / im_offset the byte offsets of the arrays
 * that `re` / `im` would point to (im_offset < 0: no imaginary part; ignored for the interleaved kinds);
 * strides stay in elements.  A MATLAB level-5 variable that is not compressed is exactly this: two column-major
 * arrays at fixed offsets (amcpy_amd/matfile.py locates them), so all_modulations.mat goes from the page cache
 * to the pinned slots through 256 KB of per-thread scratch -- without the page faults of a mapping (30 ms per
 * 436 MB variable however many threads fault) and without a host copy of the variable.  Replaces
 * scipy.io.loadmat + the slicing of feature_extraction.py:46-48,64-72.  AMCX_EIO if a read fails or the file
 * is shorter than the strides say (nothing is left in flight; the output is not written).
 */
int amcx_ctx_features18_strided_file(amcx_ctx* ctx, int32_t fd, int64_t re_offset, int64_t im_offset,
                                     int32_t kind, int64_t n_snr, int64_t n_frames, int32_t frame_size,
                                     int64_t stride_snr, int64_t stride_frame, int64_t stride_sample,
                                     float* out_host, int64_t out_row_stride, int32_t variant);
int amcx_stage_file(int32_t fd, int64_t re_offset, int64_t im_offset, int32_t kind, int64_t n_snr,
                    int64_t n_frames, int32_t frame_size, int64_t stride_snr, int64_t stride_frame,
                    int64_t stride_sample, int64_t first_unit, int64_t n_units, void* dst, int64_t dst_bytes,
                    int32_t threads, int32_t* plane_major, int32_t* inner_snr);

/*
 * Tuning of a context's upload path: threads = staging threads including the caller's (0 = keep;
 * default min(8, hardware threads); the reference's SignalConfig.num_threads maps here),
 * slot_bytes = size of one pinned staging slot (0 = keep; default 32 MiB; three are allocated),
 * round_on_device != 0: complex128 goes over PCIe as it is and is rounded by the device kernel
 * (twice the link bytes, no host arithmetic; -1 = keep).
 */
int amcx_ctx_configure(amcx_ctx* ctx, int32_t threads, int64_t slot_bytes, int32_t round_on_device);

/* what the last strided call of this context moved, and where its host time went */
typedef struct amcx_upload_stats {
  int64_t frames;
  int64_t source_bytes;     /* bytes of the container that were read */
  int64_t pcie_bytes;       /* bytes that crossed the link host -> device */
  int32_t chunks;
  int32_t threads;
  int32_t plane_major;      /* 1: planes + device transposition, 0: rows */
  int32_t from_file;       /* 1: the source was a file read by the staging threads (version 3; `reserved`, always 0, before) */
  double seconds;           /* whole call */
  double seconds_staging;   /* caller thread inside the staging copies */
  double seconds_waiting;   /* caller thread blocked on a pinned slot still being uploaded */
  double seconds_prepare;   /* before the first chunk: (re)allocation of slots and scratch */
  double seconds_tail;      /* after the last chunk was queued: feature kernel, result copy, sync */
} amcx_upload_stats;
int amcx_ctx_upload_stats(const amcx_ctx* ctx, amcx_upload_stats* out);

/*
 * The device half of the plane-major path, for callers that do their own uploads: slab_dev holds
 * n_planes sample planes, plane r = sample n0 + r of every position j < n_snr * n_frames at
 * slab_dev[r * plane_stride + j] (complex64 if src_kind == AMCX_SRC_C64, complex128 rounded here if
 * AMCX_SRC_C128).  inner_snr != 0: j = frame * n_snr + snr (Fortran order); 0: j = snr * n_frames +
 * frame.  Writes frames_dev[g * row_stride_elems + n0 + r], g = snr * n_frames + frame.
 */
int amcx_pack_planes_c64(const void* slab_dev, int32_t src_kind, int32_t n_planes, int64_t plane_stride,
                         int64_t n_snr, int64_t n_frames, int32_t inner_snr, void* frames_dev,
                         int64_t row_stride_elems, int32_t n0, void* hip_stream);

/*
 * Streaming-read ceiling probe: sums n_bytes of device memory with 16-byte
 * loads (one float per workgroup written to partial_dev, >= 4096 floats).
 * Used by bench.py to report the measured HBM read ceiling next to the
 * nominal 8 TB/s.  n_bytes must be a multiple of 16.
 */
int amcx_probe_read_bw(const void* src_dev, int64_t n_bytes, float* partial_dev,
                       void* hip_stream);

/*
 * Instruction-issue ceiling probe -- the bound that binds this path on an MI355X (the board's power cap, then VALU
 * issue: DESIGN.md section 4): one 16-wavefront workgroup per CU (four waves per SIMD, the N = 2048 kernel's
 * occupancy) runs independent v_fma_f32 on registers, no memory traffic, back to back for `seconds` (0 < seconds <=
 * 60) on hip_stream; the first half lets the clock settle, the second half is timed with HIP events.
 * *wave_instr_per_s: wavefront-instructions per second of the whole device; *clock_ghz (may be NULL): the shader
 * clock during the last launch (s_memtime cycles / s_memrealtime ticks).  Unlike the other device entries this one
 * allocates scratch and SYNCHRONISES the stream.  bench.py reports the feature kernel's own instruction rate against
 * it (roofline.secondary.measured).
 */
int amcx_probe_fma_rate(double seconds, void* hip_stream, double* wave_instr_per_s, double* clock_ghz);

/*
 * Host placement.  One process may drive every GPU of a node (the reference starts one process per modulation,
 * feature_extraction.py:89-97; here amcpy_amd.feature_extraction.DeviceFanOut runs one context per device), and a
 * context's staging threads and pinned slots belong on the socket its device hangs off.
 *
 * amcx_device_pci_bus_id: "dddd:bb:dd.f" (lower case) of visible device `device`; buf_len >= 16.
 * amcx_numa_place: host-only (no GPU needed).  Reads <sysfs_root>/bus/pci/devices/<pci_bus_id>/numa_node and
 *   .../local_cpulist (sysfs_root NULL or "" = "/sys").  *node_out = the node or -1, *n_cpus_out = how many CPUs
 *   are local (0 with node -1), the first min(n, cpus_cap) of them in cpus_out (ascending).  A platform that does
 *   not say (numa_node -1, a missing file, a malformed list) is not an error: node -1, no CPUs, nothing gets bound.
 * amcx_ctx_create does this for its device by itself (environment: AMCX_NUMA=0 turns it off, AMCX_SYSFS_ROOT names
 *   another tree); amcx_ctx_bind_cpus replaces the choice (n_cpus = 0: bind nothing; AMCX_EINVAL while a call is
 *   running on the context: bind between calls).  Bound are: the context's
 *   staging threads, and the CALLING thread for the duration of an upload large enough to use them (its own
 *   affinity mask is restored on return) -- so the pinned slots, allocated on first use inside such a call, are placed
 *   on that node too.  A binding never widens the mask the process was given (cpusets, taskset): CPUs outside it
 *   are dropped, and if none is left nothing is bound.  A thread that the CALLER's thread creates while such an upload
 *   runs (from another thread of the same Python process, say) does not inherit the narrowed mask -- only threads created
 *   BY the calling thread inside that window would, and the library creates none there: its staging threads exist before,
 *   and amcx_ctx_create warms the HIP runtime (first pinned allocation, first stream copy) so that the runtime's own
 *   helper threads are started under the creator's mask, not inside the window.
 * amcx_ctx_placement: what a context did.
 */
typedef struct amcx_placement {
  int32_t device;
  int32_t numa_node;        /* -1: unknown / unbound */
  int32_t n_cpus;           /* CPUs local to the device (or given to amcx_ctx_bind_cpus) */
  int32_t n_cpus_allowed;   /* ... of which the calling thread may use */
  int32_t first_cpu, last_cpu;
  char pci_bus_id[32];
} amcx_placement;
int amcx_device_pci_bus_id(int32_t device, char* buf, int32_t buf_len);
int amcx_numa_place(const char* sysfs_root, const char* pci_bus_id, int32_t* node_out, int32_t* cpus_out,
                    int32_t cpus_cap, int32_t* n_cpus_out);
int amcx_ctx_bind_cpus(amcx_ctx* ctx, const int32_t* cpus, int32_t n_cpus);
int amcx_ctx_placement(const amcx_ctx* ctx, amcx_placement* out);

/*
 * Consumers directly behind the path, on the device-resident
 * (rows x >=18) float32 feature matrix.
 *
 * amcx_group_stats_f32: for each of n_groups consecutive blocks of rows_per_group
 * rows, column mean and POPULATION standard deviation (ddof = 0) of the first n_cols
 * (<= 32) columns, fp64: mean_dev / std_dev are [n_groups][n_cols] doubles.
 * Replaces the per-SNR np.mean / np.std triple loop, graphics.py:50-62, and the fit
 * of StandardScaler, preprocessing.py:59-61.  The matrix is read once: every group is
 * cut into chunks (one workgroup each, ~2048 in all), a chunk's (n, sum, M2) is formed
 * from register-held tiles about each tile's own mean, and a second small launch merges
 * the chunks pairwise (Chan, Golub & LeVeque); an inf in a column gives mean +-inf and
 * std nan, as numpy's two passes do.  The chunk triples go through a workspace:
 * amcx_group_stats_f32 takes it from the stream-ordered allocator (hipMallocAsync /
 * hipFreeAsync on hip_stream: no synchronisation, but not capturable in a graph on
 * every runtime); amcx_group_stats_ws_f32 takes the caller's (at least
 * amcx_group_stats_workspace_bytes(...) bytes of device memory, contents undefined
 * afterwards; the size depends on the three arguments only, -1 for invalid ones).
 *   - checks: ranges and strides (0 <= n_groups < 2^31, rows_per_group >= 1, 1 <= n_cols <= 32, n_cols <= row_stride <= 2^20);
 *     the workspace's size (_ws, where there are groups); n_groups == 0 is AMCX_OK here, null pointers allowed; null pointers
 *     and alignment (x 4, mean and std 8, the workspace 8); a pointer on another device.
 */
int amcx_group_stats_f32(const float* x_dev, int64_t n_groups, int64_t rows_per_group,
                         int64_t row_stride, int32_t n_cols, double* mean_dev, double* std_dev,
                         void* hip_stream);
int64_t amcx_group_stats_workspace_bytes(int64_t n_groups, int64_t rows_per_group, int32_t n_cols);
int amcx_group_stats_ws_f32(const float* x_dev, int64_t n_groups, int64_t rows_per_group,
                            int64_t row_stride, int32_t n_cols, double* mean_dev, double* std_dev,
                            void* workspace_dev, int64_t workspace_bytes, void* hip_stream);

/*
 * amcx_select_scale_f32: out[r][j] = (x[r][cols[j]] - mean[j]) / scale[j], rounded to
 * float32 after each of the two operations as numpy's in-place float32 arithmetic does
 * (column pick preprocessing.py:55, StandardScaler.transform :62).  cols_dev: n_sel
 * int32 column indices (0-based, as the reference passes list(FeatureConfig.used)).
 *   - checks: ranges and strides (n_rows >= 0, n_sel >= 1, row_stride >= 1, out_stride >= n_sel, n_rows times either stride at
 *     most 2^58); n_rows == 0 is AMCX_OK here, null pointers allowed; null pointers and alignment (x, cols and out 4, mean and
 *     scale 8); a pointer on another device.
 */
int amcx_select_scale_f32(const float* x_dev, int64_t n_rows, int64_t row_stride,
                          const int32_t* cols_dev, int32_t n_sel, const double* mean_dev,
                          const double* scale_dev, float* out_dev, int64_t out_stride,
                          void* hip_stream);

/*
 * amcx_standardize_fit_transform_f32: StandardScaler().fit_transform(X[:, cols]) of
 * preprocessing.py:52-62 as three launches on hip_stream and nothing else -- no host
 * round trip, no synchronisation: statistics of all n_cols (<= 32) columns over the
 * n_rows rows (the two launches above, one group), then one launch that picks the
 * n_sel (<= 32) columns cols_host[] (HOST array of 0-based indices, passed by value),
 * turns their std into sklearn's scale_ (a column that the two-pass error bound cannot
 * tell from constant gets 1: var <= n eps var + (n mean eps)^2, sklearn >= 0.24
 * _is_constant_feature), writes mean_dev[n_sel] / scale_dev[n_sel] (doubles) and
 * out_dev[r][j] with the two float32 roundings of amcx_select_scale_f32.
 * workspace_dev: at least amcx_standardize_workspace_bytes(n_rows, n_cols) bytes.
 *   - checks: ranges and strides (n_rows >= 0, 1 <= n_sel <= 32, 1 <= n_cols <= 32, cols_host there and every index a column,
 *     row_stride >= n_cols, out_stride >= n_sel, n_rows times either at most 2^58; where there are rows, row_stride <= 2^20 and
 *     n_rows < 2^41); the workspace's size (where there are rows); n_rows == 0 is AMCX_OK here, null pointers allowed; null
 *     pointers and alignment (x and out 4, mean and scale 8, the workspace 8); a pointer on another device.
 */
int64_t amcx_standardize_workspace_bytes(int64_t n_rows, int32_t n_cols);
int amcx_standardize_fit_transform_f32(const float* x_dev, int64_t n_rows, int64_t row_stride,
                                       int32_t n_cols, const int32_t* cols_host, int32_t n_sel,
                                       float* out_dev, int64_t out_stride, double* mean_dev,
                                       double* scale_dev, void* workspace_dev, int64_t workspace_bytes,
                                       void* hip_stream);

/*
 * ABI 8.  CLASSIFICATION: the reference's AMCClassifier in eval() mode (nn_model.py:28-75: Linear, BatchNorm1d,
 * activation, Dropout (identity in eval), ..., Linear, Softmax) and the `model(x_t).argmax(1)` plus accuracy count of
 * its evaluate_by_snr (nn_model.py:250-259), as ONE launch over the device-resident (n_rows x n_cols) float32 matrix.
 *
 * The network is n_linear (1 ... 6) dense layers of widths widths_host[0 .. n_linear] (n_linear + 1 entries, each
 * 1 ... 32; widths_host[0] == n_sel inputs, widths_host[n_linear] classes), the activation (AMCX_ACT_*) between them
 * and softmax behind the last.  params_dev is the PACKED PARAMETER BLOCK, float32, no padding, amcx_mlp_params_floats
 * floats in all (sum over layers of out * in + out; -1 for an invalid shape): for layer l = 0 ... n_linear - 1
 *     W'[out][in] row-major (out = widths[l + 1], in = widths[l]), then b'[out].
 * BATCHNORM FOLD (the caller's, in float64, rounded once to float32): a Linear (W, b) followed by an eval-mode
 * BatchNorm1d (gamma, beta, running mean mu, running variance var, eps = 1e-5) is the one dense layer
 *     g = gamma / sqrt(var + eps);   W'[o][k] = W[o][k] * g[o];   b'[o] = (b[o] - mu[o]) * g[o] + beta[o];
 * a Linear without BatchNorm is W' = W, b' = b.
 *
 * Per row r:  h[j] = float(float(x[r][cols_host[j]] - mean_dev[j]) / scale_dev[j]), the two float32 roundings of
 * amcx_select_scale_f32 (mean / scale: n_sel doubles in DEVICE memory, e.g. as amcx_standardize_fit_transform_f32 left
 * them -- no host round trip; both null: the rows are standardised already, columns are picked only; one null:
 * AMCX_EINVAL).  Every layer: out[o] = b'[o] + sum_k W'[o][k] h[k], float32 FMAs in the order k = 0 ... in - 1, so a
 * row's result does not depend on how rows are batched.  Softmax subtracts the row maximum; the label is the first
 * maximum, as torch.argmax.
 *
 * Outputs, each pointer may be null: labels_dev[r] (int32); probs_dev[r * probs_stride + c] (float32,
 * probs_stride >= classes); counts_dev[group][classes + 1] (int64), groups being consecutive blocks of rows_per_group
 * rows (amcx_group_stats_f32's convention; n_rows must be a whole number of groups; rows_per_group 0 only with
 * counts_dev null).  counts_dev is zeroed by the call itself (a small launch on hip_stream ahead of the classifier's);
 * nothing is allocated, so the call can be captured in a graph.
 * NaN RULE, a deliberate difference from the reference: a row whose probabilities are not all finite (a NaN feature of
 * a constant frame, a column a feature subset left NaN, an inf) keeps its probabilities as they come out (NaN), gets
 * label -1 and is counted in the extra last bin, counts[group][classes].  The reference's argmax answers class 0
 * (BPSK) for such a row.
 * n_rows == 0 is AMCX_OK and a no-op.  Arguments are checked before any HIP call.  amcx_mlp_kernel_name: the kernel
 * that runs for this shape (host-only).
 *   - checks: ranges and strides (1 <= n_cols <= 32, n_rows >= 0, row_stride >= n_cols, the shape, n_sel == widths_host[0], the
 *     activation, mean and scale both or neither, every index a column, probs_stride >= classes where probs_dev is given,
 *     n_rows times either stride at most 2^58, whole groups); n_rows == 0 is AMCX_OK here, null pointers allowed; null pointers
 *     (x, params) and alignment (x, params, labels and probs 4, mean, scale and counts 8); a pointer on another device; with
 *     no output asked for the call is AMCX_OK then, and launches nothing.
 */
#define AMCX_ACT_RELU 0
#define AMCX_ACT_TANH 1
#define AMCX_ACT_SIGMOID 2
int64_t amcx_mlp_params_floats(const int32_t* widths_host, int32_t n_linear);
int amcx_mlp_classify_f32(const float* x_dev, int64_t n_rows, int64_t row_stride, int32_t n_cols,
                          const int32_t* cols_host, int32_t n_sel, const double* mean_dev, const double* scale_dev,
                          const float* params_dev, const int32_t* widths_host, int32_t n_linear, int32_t activation,
                          int32_t* labels_dev, float* probs_dev, int64_t probs_stride, int64_t rows_per_group,
                          int64_t* counts_dev, void* hip_stream);
int amcx_mlp_kernel_name(const int32_t* widths_host, int32_t n_linear, char* buf, int32_t buf_len);

/*
 * ABI 16.  FIXED-POINT DEPLOYMENT of the network amcx_mlp_classify_f32 runs: the reference's `quantize` stage
 * (nn_quantization.py) turns a trained model into 16-bit integers for a microcontroller.  Two device entries stand behind the
 * export (amcpy_amd/quantize.py): the calibration of every layer's range over all rows, and the integer network itself, so
 * that what the 16-bit network answers, and where it saturates, is known before it is on the board.  Both take the rows, the
 * column pick, the scaler and the shape exactly as amcx_mlp_classify_f32 does, launch on hip_stream, allocate nothing, never
 * synchronise, and zero what they need zeroed with a launch of their own: they can be captured in a graph.
 *
 * amcx_mlp_range_f32.  params_dev: the float32 packed block.  h and every layer's sums are amcx_mlp_classify_f32's, bit for
 * bit (the two float32 roundings of the scaler; bias first, then one float32 FMA per k = 0 ... in - 1); between the layers
 * AMCX_ACT_RELU or AMCX_ACT_NONE (nothing: the chain the reference calibrates on); tanh and sigmoid are AMCX_EINVAL.
 * ranges_dev: float32 [n_linear + 1][2], (min, max) of the standardised input over the n_sel columns, then of every layer's
 * PRE-activation values over its outputs, over all rows that count; skipped_dev: one int64, the number of rows one of whose
 * inputs or pre-activation values is not finite -- such a row contributes nothing to any range.  Min and max do not depend on
 * the order they are taken in: the result is exact.  A zero is reported as +0.  With no row that counts a range stays
 * (+inf, -inf).  Both pointers are required.
 *   - checks: the limits of amcx_mlp_classify_f32 (rows, strides, columns, shape, mean and scale both or neither), the
 *     activation; n_rows == 0 is AMCX_OK here, null pointers allowed, nothing written; null pointers (x, params, ranges,
 *     skipped) and alignment (x, params and ranges 4, mean, scale and skipped 8); a pointer on another device.
 *
 * amcx_mlp_classify_q15.  params_dev: the packed block as int16, the float block's layout (per layer W[out][in] row-major,
 * then b[out]; amcx_mlp_q15_params_shorts values, -1 for an invalid shape).  frac_input, and per layer frac_weights_host[l],
 * frac_biases_host[l], frac_outputs_host[l] (host arrays of n_linear entries): the fractional bits Nw, Nb, No of the Q-format
 * each int16 stands in, 0 ... 15 each.  THE ARITHMETIC, all of it exact integers (Na starts as frac_input):
 *   input   a[k] = int(rint(clamp(h[k] * 2^Na, -16384, 16383))), h the standardised float32 value, the product and the clamp
 *           in float32 (a power of two: the product is exact), rint to nearest-even.  (The reference's table Qm.n, m + n = 15,
 *           holds [-2^(m-1), 2^(m-1) - 2^-n]: half of what 16 bits hold, and this is its clamp.)  A row with a non-finite h
 *           gets label -1, zeros for logits, is counted in the extra last bin and takes no further part.
 *   layer   P = Nw + Na;  acc = sum_k W[o][k] * a[k] + (b[o] << (P - Nb));  s = P - No;  v = (acc + 2^(s-1)) >> s, an
 *           arithmetic shift, so a half rounds up;  out = clamp(v, -32768, 32767);  a hidden layer then takes max(out, 0);
 *           Na becomes No.  The call is AMCX_EINVAL unless P >= Nb and P > No in every layer.
 * The sums are exact for EVERY int16 block and every int16 activation (acc can pass 2^35: it is kept in 64 bits).  Relu only:
 * any other activation is AMCX_EINVAL.
 * Outputs, each pointer may be null: labels_dev[r] (int32), the first maximum of the last layer's int16 values;
 * logits_dev[r * logits_stride + c] (int16, logits_stride >= classes); counts_dev[group][classes + 1] (int64) in
 * amcx_mlp_classify_f32's convention; saturated_dev[n_linear + 1] (int64), counted over the rows that have a label:
 * [0] the input values the clamp changed, [l] the outputs of layer l with v > 32767 and, for the last layer, also those with
 * v < -32768 -- the clips that change a result (below -32768 in a hidden layer relu gives 0 either way).  The call zeroes
 * counts_dev and saturated_dev itself.
 *   - checks: the limits of amcx_mlp_classify_f32, the activation, the format arrays and every format's range and the two
 *     shifts, logits_stride >= classes where logits_dev is given, whole groups; n_rows == 0 is AMCX_OK here, null pointers
 *     allowed; null pointers (x, params) and alignment (x and labels 4, params and logits 2, mean, scale, counts and saturated
 *     8); a pointer on another device; with no output asked for the call is AMCX_OK then, and launches nothing.
 * amcx_kernel_name_mlp_q15 (host-only): 0 the integer network's kernel, 1 the range kernel, 2 its initialising launch; NULL
 * for any other number.
 */
#define AMCX_ACT_NONE 3      /* amcx_mlp_range_f32 only */
int amcx_mlp_range_f32(const float* x_dev, int64_t n_rows, int64_t row_stride, int32_t n_cols, const int32_t* cols_host,
                       int32_t n_sel, const double* mean_dev, const double* scale_dev, const float* params_dev,
                       const int32_t* widths_host, int32_t n_linear, int32_t activation, float* ranges_dev, int64_t* skipped_dev,
                       void* hip_stream);
int64_t amcx_mlp_q15_params_shorts(const int32_t* widths_host, int32_t n_linear);
int amcx_mlp_classify_q15(const float* x_dev, int64_t n_rows, int64_t row_stride, int32_t n_cols, const int32_t* cols_host,
                          int32_t n_sel, const double* mean_dev, const double* scale_dev, const int16_t* params_dev,
                          const int32_t* widths_host, int32_t n_linear, int32_t activation, int32_t frac_input,
                          const int32_t* frac_weights_host, const int32_t* frac_biases_host, const int32_t* frac_outputs_host,
                          int32_t* labels_dev, int16_t* logits_dev, int64_t logits_stride, int64_t rows_per_group,
                          int64_t* counts_dev, int64_t* saturated_dev, void* hip_stream);
const char* amcx_kernel_name_mlp_q15(int32_t which);

/*
 * ABI 16.1.  TRAINING of the network amcx_mlp_classify_f32 runs: the reference's `train` stage (nn_model.train_model) on the
 * device, ONE workgroup of 256 threads per model and n_models workgroups per launch (amcpy_amd/csrc/amcx_mlp_train_kernel.h).
 * A call runs steps step0 ... step0 + n_steps - 1 of ONE epoch for every model, on hip_stream; it allocates nothing, never
 * synchronises and can be captured in a graph.  The rows, columns, scaler and shape are amcx_mlp_classify_f32's.
 *
 * THE NETWORK, in train mode.  Per hidden layer l (0-based): z = W a + b; where bit l of bn_mask is set BatchNorm1d over the
 * batch (batch mean, biased variance, eps 1e-5; running mean / variance updated with momentum 0.1, the running variance from
 * the unbiased variance; then gamma, beta); the activation; dropout (a kept value times keep_scale).  The last layer is
 * z = W a + b and p = softmax(z).  A bit of bn_mask at or above n_linear - 1 is AMCX_EINVAL.  THE LOSS is the reference's,
 * CrossEntropyLoss on the softmax OUTPUT: q = softmax(p), a row's loss -log q[y], dp = (q - onehot(y)) / rows,
 * dz = p * (dp - sum_j p_j dp_j).  THE OPTIMIZERS are torch's with torch's defaults, in float32: AMCX_OPT_RMSPROP (alpha 0.99,
 * eps 1e-8) and AMCX_OPT_ADAM (betas 0.9 / 0.999, eps 1e-8, bias correction from the model's step count).
 *
 * ROWS.  y_dev: int32 [n_rows], a row's class (one outside 0 ... classes - 1 matches no class).  idx_dev: int32, the epoch's
 * order, n_idx row numbers per model; idx_model_stride is 0 when every model takes the same order, else the distance in
 * elements between two models' orders (>= n_idx).  Step s takes idx[s * batch ... min((s + 1) * batch, n_idx) - 1]: the ragged
 * last batch has n_idx mod batch rows, and n_idx mod batch == 1 is AMCX_EINVAL (a BatchNorm of one row).  batch: 2 ... 256.  An
 * index outside 0 ... n_rows - 1 is the caller's error; the kernel reads the nearest row instead.
 *
 * THE STATE BLOCK.  state_dev: float32 [n_models][amcx_mlp_train_state_floats(widths, n_linear, bn_mask, optimizer)], per model
 *   [0, P)                     the packed parameter block of amcx_mlp_params_floats: per layer W[out][in] row-major, then b[out];
 *   [P, P + A)                 per BatchNorm, ascending layers: gamma[out], then beta[out]                    (T = P + A trainable)
 *   [T, T + R)                 per BatchNorm: running_mean[out], then running_var[out]                         (R = A)
 *   [T + R + s T, ... + T)     optimizer slot s of trainable value i at + i: rmsprop one slot (square_avg), adam two (exp_avg,
 *                              then exp_avg_sq).
 * steps_dev: int64 [n_models], the steps a model has taken (torch's num_batches_tracked and the optimizers' `step`); the call
 * adds n_steps.  Nothing else carries over from one call to the next: an epoch cut into calls anywhere gives the bits of one call.
 * ws_dev: float32 [n_models][amcx_mlp_train_workspace_floats(widths, n_linear, batch)], 16-byte aligned, scratch: what backward
 * needs of forward (a CU's LDS does not hold it for the largest shape); its contents mean nothing between calls.
 *
 * HYPERPARAMETERS, host arrays of n_models entries: lr_host (finite), drop_threshold_host, keep_scale_host (finite), seed_host.
 * THE DROPOUT MASK is part of the contract: Philox4x32-10 with the key (seed low word, seed high word); the counter
 * (t mod 2^32, hidden layer l, row in the batch r, o / 4) gives the four words of units 4 (o / 4) ... + 3, t being the model's
 * step count BEFORE the step; a unit is kept iff its word >= drop_threshold.  The caller computes drop_threshold = rint(p 2^32)
 * and keep_scale = float32(1 / (1 - p)); with drop_threshold 0 (keep_scale 1) the bits are those of a run without dropout.
 *
 * history_dev: float64 [n_models][2].  The call ADDS, step by step, the batch's summed row losses to [m][0] and the number of
 * rows whose argmax p (first maximum) is y to [m][1], rows in order: bit-reproducible, and the same however the epoch is cut.
 *
 *   - checks, in the order of every launching entry: the limits of amcx_mlp_classify_f32, the activation, bn_mask, the optimizer,
 *     batch, n_models >= 1, n_steps >= 0, step0 >= 0, 0 <= n_idx < 2^31, idx_model_stride, the ragged-batch rule, step0 * batch <
 *     n_idx and the last step inside the epoch when n_steps > 0, the host arrays present, every lr and keep_scale finite;
 *     n_steps == 0 or n_rows == 0 is AMCX_OK here and writes nothing; then null pointers, alignment (4; 8 for mean, scale,
 *     history and steps; 16 for ws) and a pointer on another device.
 * amcx_mlp_train_state_floats / amcx_mlp_train_workspace_floats: -1 for an invalid shape (or batch).
 * amcx_kernel_name_mlp_train (host-only): the kernel of an (activation, optimizer), a static string; (-1, -1): the launch that
 * carries the hyperparameters to the device; NULL otherwise.
 */
int amcx_abi_minor(void);      /* AMCX_ABI_MINOR of the library */
#define AMCX_OPT_RMSPROP 0
#define AMCX_OPT_ADAM 1
int64_t amcx_mlp_train_state_floats(const int32_t* widths_host, int32_t n_linear, uint32_t bn_mask, int32_t optimizer);
int64_t amcx_mlp_train_workspace_floats(const int32_t* widths_host, int32_t n_linear, int32_t batch);
int amcx_mlp_train_f32(const float* x_dev, int64_t n_rows, int64_t row_stride, int32_t n_cols, const int32_t* cols_host,
                       int32_t n_sel, const double* mean_dev, const double* scale_dev, const int32_t* y_dev, const int32_t* idx_dev,
                       int64_t n_idx, int64_t idx_model_stride, const int32_t* widths_host, int32_t n_linear, int32_t activation,
                       uint32_t bn_mask, int32_t optimizer, int32_t batch, int32_t n_models, float* state_dev, int64_t* steps_dev,
                       float* ws_dev, const float* lr_host, const uint32_t* drop_threshold_host, const float* keep_scale_host,
                       const uint64_t* seed_host, int64_t step0, int32_t n_steps, double* history_dev, void* hip_stream);
const char* amcx_kernel_name_mlp_train(int32_t activation, int32_t optimizer);

/*
 * ABI 16.2.  THE WAVEFORM GENERATOR: n_rows rows of row_samples complex64 samples of a linearly modulated signal -- symbols drawn
 * by Philox4x32-10, a pulse at U / V samples per symbol (up / down), a carrier, white Gaussian noise -- in ONE launch on
 * hip_stream (amcpy_amd/csrc/amcx_synth_kernel.h).  It allocates nothing, never synchronises and can be captured in a graph; no
 * atomics, no workgroup waits for another.  A row is one frame or one long stream.  r = row_index0 + f is the ABSOLUTE row of
 * the call's row f, n = sample_index0 + i the ABSOLUTE sample of its sample i: a call can begin anywhere.
 *
 *   key              = (seed low word, seed high word)                 Philox4x32-10, the generator of the dropout mask above
 *   counter(s, j, r) = (j & 0xFFFFFFFF, (s << 28) | (j >> 32), r low word, r high word)      stream s = 0 row, 1 symbols, 2 noise
 *   row words        W = Philox(counter(0, 0, r))
 *     carrier phase  phase0_r = flags & AMCX_SYNTH_RANDOM_PHASE  ? (uint64)W[0] << 32 : 0
 *     carrier step   step_r   = phase_step + (uint64)((int64)(int32)W[1] * (int64)cfo_max)   mod 2^64, in 2^-64 cycles per sample
 *                               cfo_max: in 2^-33 cycles per sample, the largest offset a row draws; 0 = none
 *     timing         tau_r    = flags & AMCX_SYNTH_RANDOM_TIMING ? mulhi32(W[2], U) : tau0    0 <= tau < U
 *   symbol k >= 0    a[k] = table[mulhi32(Philox(counter(1, k >> 2, r))[k & 3], order)]      table_c64_dev: `order` complex64 points
 *   pulse            t_n = n V + tau_r,  p_n = t_n mod U,  k_n = (P - 1) + floor(t_n / U),  P = ceil(T / U),  T = n_taps
 *                    s[n] = sum_{q >= 0, p_n + q U < T} g[p_n + q U] * a[k_n - q]             g = taps_dev, at U samples per symbol
 *                    one product, then one FMA per component in ascending q: amcx_resample's order with L = U, D = V
 *   carrier          v[n] = s[n] * exp(+2 pi j phi / 2^64), phi = phase0_r + n * step_r: the down-converter's mixer, the same bits
 *                    (phi < 2^32 skips the product)
 *   noise            X = Philox(counter(2, n >> 1, r));  w1 = X[2 (n & 1)],  w2 = X[2 (n & 1) + 1]
 *                    u = ((w1 >> 8) + 1) * 2^-24          in (0, 1], exact in float32
 *                    z[n] = (sigma_g * sqrt(-ln u)) * exp(2 pi j w2 / 2^32)                   the same mixer; E|z|^2 = sigma_g^2
 *                    sigma_g = sigma_dev[f / frames_per_group], f the row's index IN THE CALL
 *   out[f, i]        = (v.re + z.re, v.im + z.im)         one float32 addition per component; at out_c64_dev + f row_stride + i
 *
 * order == 0 is the noise class: s is exactly +0 + 0j, no symbol is drawn, table_c64_dev is not read (and may be NULL).
 * sigma_g == 0 gives out == v, the signed zeros of v kept.  No gain is applied anywhere: a pulse with sum g^2 = U and a table of
 * unit power give unit signal power, SNR = 1 / sigma^2.  THE LOGARITHM is the device library's float32 logf and the noise is held
 * to a derived bound (tests/synth_ref.py), every integer above exactly.  sigma is read on the device, where the host cannot see
 * it: a NaN or negative sigma is not refused, it propagates into the row.
 *
 * POSITION INDEPENDENCE.  The bits of out[f, i] depend on the seed, r, n, the row parameters, the taps, the table and sigma_g,
 * and not on the call's cut, the tile, the grid, the lane, row_stride or n_rows: a data set made in any number of calls over
 * rows, or a stream made in chunks of any length, odd lengths included, equals one call bit for bit.
 *
 *   - limits: 0 <= order <= 256, 1 <= up <= 256, 1 <= down <= 4096, 1 <= n_taps <= 4096; 0 <= tau0 < up, no flag but the two;
 *     1 <= row_samples, 0 <= sample_index0, sample_index0 + row_samples < 2^40; 0 <= n_rows, row_stride >= row_samples,
 *     n_rows * row_stride <= 2^58; frames_per_group >= 1; every sigma read a finite float32 >= 0 (not checked, see above)
 *   - checks, in the order of every launching entry: the limits in that order; n_rows == 0 is AMCX_OK here and writes nothing;
 *     then null pointers (the table only where order > 0), alignment (out 8; taps, table and sigma 4) and a pointer on another
 *     device.  Ordinary vector stores only.
 * amcx_synth_plan (host-only): samples per tile, bytes of LDS and the most workgroups of the persistent grid for a shape; each
 * pointer may be NULL.  amcx_kernel_name_synth (host-only): the kernel's name, a static string.
 */
#define AMCX_SYNTH_RANDOM_PHASE 1u
#define AMCX_SYNTH_RANDOM_TIMING 2u
int amcx_synth_plan(int32_t order, int32_t n_taps, int32_t up, int32_t down, int32_t* tile_outputs, int32_t* lds_bytes,
                    int32_t* max_workgroups);
int amcx_synth_c64(uint64_t seed, uint64_t row_index0, int64_t sample_index0, int64_t n_rows, int64_t row_samples,
                   int64_t row_stride, const void* table_c64_dev, int32_t order, const float* taps_dev, int32_t n_taps, int32_t up,
                   int32_t down, int32_t tau0, uint64_t phase_step, uint32_t cfo_max, uint32_t flags, const float* sigma_dev,
                   int64_t frames_per_group, void* out_c64_dev, void* hip_stream);
const char* amcx_kernel_name_synth(void);

/*
 * ABI 16.2.1.  THE FADING MULTIPATH CHANNEL: n_rows rows of complex64, each through its own time-varying tapped delay line, in
 * ONE launch on hip_stream (amcpy_amd/csrc/amcx_channel_kernel.h).  A path's gain is a sum-of-sinusoids Rayleigh process (Jakes
 * Doppler spectrum) plus an optional line-of-sight term (Rician); optionally the launch adds the generator's white noise.  It
 * allocates nothing, never synchronises and can be captured in a graph; no atomics, no workgroup waits for another.
 * r = row_index0 + f is the ABSOLUTE row of the call's row f, n = sample_index0 + i the ABSOLUTE output sample of its sample i.
 * L = n_paths, S = n_sinusoids, B = 2^interp_log2, H = the largest delay: the history.  A row of the input holds
 * row_samples + H samples and output i reads input i + H - delay_l: the down-converter's convention.
 *
 *   path record      16 bytes, a HOST array of L, passed to the kernel by value (the host sees and checks every delay):
 *                    int32 delay (samples), float diffuse_gain (of the sum of sinusoids), float los_gain (of the line of sight),
 *                    int32 los_doppler_q31 (the line of sight's Doppler in 2^-31 of the Doppler unit)
 *   key, counter     the generator's (ABI 16.2), with the new stream number 3
 *   sinusoid (l, s)  X = Philox(counter(3, 32 l + s, r));  phase0_ls = (uint64)X[0] << 32
 *                    c = the real part of the mixer's value at the angle X[1]: the cosine of a uniform arrival angle, its float32 bits
 *                    ci = (int64)(c * 2^31)          the product is exact in float32, the conversion truncates toward zero
 *                    step_ls = ci * doppler_max      in int64, used mod 2^64.  doppler_max (uint32): the maximum Doppler is
 *                                                    doppler_max / 2^33 cycles per sample, the unit of cfo_max
 *   line of sight l  XL = Philox(counter(3, 512 + l, r));  phase0 = flags & AMCX_CHANNEL_RANDOM_PHASE ? (uint64)XL[0] << 32 : 0
 *                    step = (int64)los_doppler_q31 * doppler_max
 *   node gains       at the absolute sample k B:
 *                    d = sum over s = 0 ... S - 1, ascending, of mixer(top 32 bits of phase0_ls + k B step_ls): plain float32
 *                        additions per component, from the s = 0 value
 *                    w = the line of sight's mixer value at k B
 *                    G_l[k] = fma(los_gain, w, diffuse_gain * d)                               per component
 *   sample gain      k = n >> interp_log2,  f = (float)(n & (B - 1)) * 2^-interp_log2
 *                    c_l[n] = fma(f, G_l[k + 1] - G_l[k], G_l[k])                              per component
 *                    (interp_log2 = 0: the closed form at every sample)
 *   output           x_l = in[f, i + H - delay_l];  paths in ascending l.  The first path:
 *                      acc.re = fma(c.re, x.re, -(c.im x.im)),  acc.im = fma(c.re, x.im, c.im x.re)
 *                    every later path, in this order:
 *                      acc.re = fma(c.re, x.re, acc.re);  acc.re = fma(-c.im, x.im, acc.re)
 *                      acc.im = fma(c.re, x.im, acc.im);  acc.im = fma(c.im, x.re, acc.im)
 *                    out[f, i] = acc with the generator's noise added: its stream-2 words of (r, n), sigma_g =
 *                    sigma_dev[f / frames_per_group] read on the device as the generator reads it; sigma_dev NULL: no noise
 *
 * POSITION INDEPENDENCE.  Nothing above depends on the call's cut, the tile, the grid, the lane or the strides: rows cut into
 * calls, or a stream cut into chunks of any length (each with the H samples in front of it), equal one call bit for bit.
 * Non-finite gains are not refused: they propagate.
 *
 *   - limits: 1 <= n_paths <= 16, 1 <= n_sinusoids <= 32, 0 <= interp_log2 <= 16, 0 <= delay <= 1024, no flag but the one;
 *     1 <= row_samples, 0 <= sample_index0, sample_index0 + row_samples < 2^40; 0 <= n_rows, in_row_stride >= row_samples + H,
 *     out_row_stride >= row_samples, n_rows times either stride <= 2^58; frames_per_group >= 1; at most 2^31 - 1 (row, tile) items
 *   - checks, in the order of every launching entry: the limits (paths_host NULL among them); n_rows == 0 is AMCX_OK here and
 *     writes nothing; then null pointers (in, out), alignment (in and out 8, sigma 4), a pointer on another device, and the
 *     byte ranges of input and output, which must not overlap: the kernel reads neighbours of the sample it writes.
 *     Ordinary vector stores only.
 * The plan entry (host-only): outputs per tile and bytes of LDS for a shape; each pointer may be NULL.  The name entry
 * (host-only): the kernel's name, a static string.  amcx_abi_patch: AMCX_ABI_PATCH of the library.
 */
#define AMCX_CHANNEL_RANDOM_PHASE 1u
#define AMCX_CHANNEL_MAX_PATHS 16
#define AMCX_CHANNEL_MAX_SINUSOIDS 32
#define AMCX_CHANNEL_MAX_DELAY 1024
int amcx_abi_patch(void);
int amcx_channel_plan(int32_t n_paths, int32_t n_sinusoids, int32_t interp_log2, int32_t max_delay, int32_t* tile_outputs,
                      int32_t* lds_bytes);
int amcx_channel_c64(uint64_t seed, uint64_t row_index0, int64_t sample_index0, int64_t n_rows, int64_t row_samples,
                     const void* in_c64_dev, int64_t in_row_stride, const void* paths_host, int32_t n_paths, int32_t n_sinusoids,
                     int32_t interp_log2, uint32_t doppler_max, uint32_t flags, const float* sigma_dev, int64_t frames_per_group,
                     void* out_c64_dev, int64_t out_row_stride, void* hip_stream);
const char* amcx_kernel_name_channel(void);

/*
 * ABI 16.2.2.  THE CONTINUOUS-PHASE GENERATOR: n_rows rows of row_samples complex64 samples of exp(j Phi[n]) -- FSK, MSK, GMSK --
 * in ONE launch on hip_stream (amcpy_amd/csrc/amcx_synth_cpm_kernel.h).  Phi is a running sum over every symbol so far, kept in
 * uint32 arithmetic mod 2^32 in units of 2^-32 turn, the units the mixer reads: integer sums are associative, so any order gives
 * the same bits.  It allocates nothing, never synchronises and can be captured in a graph; no atomics, no workgroup waits for
 * another.  Everything named here that ABI 16.2 defines keeps its definition from amcx_synth_c64: the key and the counters, the
 * row words (phase0_r, step_r, tau_r), t_n, p_n, k_n, P, the symbol draw idx_j of stream 1 (a row of order M draws the indices a
 * linear row of order M draws), the noise words of stream 2, sigma_g, r and n absolute.
 *
 *   symbol           alpha_j = 2 idx_j - (order - 1)                 an integer of -(M - 1) ... M - 1 in steps of 2
 *   phase pulse      Qc(i) = phase_taps_dev[i] for 0 <= i < T = n_taps,  phase_full for i >= T;  at U samples per symbol
 *   phase            Phi_r[n] = sum_{j = 0 ... k_n} alpha_j * Qc(t_n - (j - P + 1) U)                mod 2^32
 *                    computed as phase_full * A(k_n - cnt_n + 1) + sum_{q < cnt_n} alpha[k_n - q] * phase_taps[p_n + q U],
 *                    cnt_n the taps of phase p_n (the q with p_n + q U < T), A(K) = sum_{j < K} alpha_j
 *   out[f, i]        = the generator's carrier and noise on (1, 0) at phi = phase0_r + n step_r + ((uint64)Phi_r[n] << 32)
 *
 * The signal has unit amplitude: sigma and SNR = 1 / sigma^2 keep the generator's meaning.
 * THE CARRIED SUM.  acc_in_dev[f] = A(K0) mod 2^32, K0 = floor(sample_index0 V / U): it does not depend on the drawn timing
 * (the kernel adds alpha_K0 itself where the row's first window begins one symbol later).  It may be NULL only where
 * sample_index0 == 0 (A(0) = 0).  acc_out_dev, where not NULL, gets A(floor((sample_index0 + row_samples) V / U)) per row: the
 * acc_in of the call that continues the rows.  With a true acc_in the bits of out[f, i] depend on (seed, r, n), the row
 * parameters, the pulse and sigma_g alone -- ABI 16.2's position independence with one word of state per row.
 * A row is cut into `segments` runs of whole tiles, one workgroup each, which changes no bit; 0 leaves the cut to the plan.
 *
 *   - limits: 2 <= order <= 256; up, down, n_taps, tau0, flags, row_samples, sample_index0, n_rows, row_stride and
 *     frames_per_group as amcx_synth_c64; 0 <= segments <= 64; at most 2^31 - 1 (row, segment) items
 *   - checks, in the order of every launching entry: the limits in that order; n_rows == 0 is AMCX_OK here and writes nothing;
 *     then null pointers (out, phase_taps, sigma; acc_in where sample_index0 > 0), alignment (out 8, the others 4), a pointer
 *     on another device, and the two acc arrays, which must not overlap.  Ordinary vector stores only.
 * amcx_synth_cpm_plan (host-only): samples per tile, bytes of LDS and the segments a call with segments = 0 cuts a row into (1
 * where the rows alone fill the device, else about two workgroups per compute unit, never more than the row's tiles or 64);
 * each pointer may be NULL.  amcx_kernel_name_synth_cpm (host-only): the kernel's name, a static string.
 */
int amcx_synth_cpm_plan(int32_t n_taps, int32_t up, int32_t down, int64_t n_rows, int64_t row_samples, int32_t* tile_outputs,
                        int32_t* lds_bytes, int32_t* segments);
int amcx_synth_cpm_c64(uint64_t seed, uint64_t row_index0, int64_t sample_index0, int64_t n_rows, int64_t row_samples,
                       int64_t row_stride, int32_t order, const uint32_t* phase_taps_dev, int32_t n_taps, uint32_t phase_full,
                       int32_t up, int32_t down, int32_t tau0, uint64_t phase_step, uint32_t cfo_max, uint32_t flags,
                       const float* sigma_dev, int64_t frames_per_group, const uint32_t* acc_in_dev, uint32_t* acc_out_dev,
                       int32_t segments, void* out, void* hip_stream);
const char* amcx_kernel_name_synth_cpm(void);

/*
 * ABI 16.2.3.  BLIND CARRIER RECOVERY: n_rows rows of n complex64 samples to one 32-byte record per row -- power, gain, the
 * carrier's offset and phase as the down-converter's integer words, a quality figure -- and, where out is given, the row with
 * gain, frequency and phase taken out, in ONE launch on hip_stream (amcpy_amd/csrc/amcx_carrier_kernel.h).  The estimator raises
 * the normalised row to the M-th power (M = order: 2 for BPSK, 4 for QPSK, 8 for 8PSK, 1 for a bare carrier), transforms it and
 * interpolates the largest line inside a bounded range.  It allocates nothing, never synchronises and can be captured in a
 * graph; no atomics, no workgroup waits for another.  N = n = 2^lg, M = 2^lm, sb = search_bins; tests/carrier_ref.py restates
 * every line in numpy float32, operation by operation.
 *
 *   the record       32 bytes, 8-byte aligned: int64 phase_step, uint32 phase0, int32 bin, float frac, float power, float gain,
 *                    float quality
 *   power            q[n] = fma(im, im, re re);  THE TREE: q'[i] = q[2 i] + q[2 i + 1] until one value is left (an order that
 *                    depends on N alone);  power = tree * (1 / N), exact
 *   gain             1.0f / sqrtf(power), root and quotient correctly rounded.  A power of 0, NaN or inf: gain 0, a record of
 *                    zeros beside power, an output row of zeros
 *   u, z             u[n] = (gain re, gain im);  z = u, squared lm times with mul(z, z),
 *                    mul(d, w) = (fma(d.re, w.re, -(d.im w.im)), fma(d.re, w.im, d.im w.re))  -- the spectrogram's product.
 *                    (u has unit power, so the eighth power stays inside float32 whatever the level of x.)
 *   Z                THE OPERATION SEQUENCE of the spectrogram (ABI 15, amcx_psd_kernel.h) on z, no window product;
 *                    P[k] = fma(Z.im, Z.im, Z.re Z.re)
 *   bin              over the SIGNED k of -sb ... sb (Z[k] is Z[k mod N]): the key is P[k], or -1 where P[k] is NaN; bin has the
 *                    largest key, ties to the lowest signed k.  The bound matters beyond speed: under a root-raised-cosine
 *                    pulse z also has lines one symbol rate away.
 *   frac             a, b, c = Z[bin - 1], Z[bin], Z[bin + 1];  num = c - a;  den = (b - a) + (b - c), per component;
 *                    frac = -(fma(num.im, den.im, num.re den.re) / fma(den.im, den.im, den.re den.re)), 0 unless |frac| <= 0.5
 *   phase_step       F = (int64)rintf(frac 2^31);  step_M = bin 2^(64 - lg) + F 2^(33 - lg);  phase_step = step_M >> lm, an
 *                    ARITHMETIC shift: the carrier's offset in the down-converter's unit, 2^-64 cycle per sample
 *   phase0           w = (int64)rintf((atan2f(b.im, b.re) * (float)(1 / 2 pi)) * 2^32)   the device library's atan2f;
 *                    theta_M = (uint32)(w - ((F (N - 1)) >> lg)), the shift arithmetic;  phase0 = theta_M >> lm, a LOGICAL shift,
 *                    in 2^-32 cycle.  THE M-FOLD AMBIGUITY: the M-th power cannot tell the carrier's phase from that phase plus
 *                    any multiple of 1 / M cycle; phase0 is the one of those M equivalent phases in [0, 1 / M).  After recovery
 *                    a constellation stands upright up to one of its own M-fold rotations.
 *   quality          P[bin] / ((float)N * tree(|z|^2)), |z|^2 formed as q is: 1 for a tone on a bin, of the order of 1 / N for
 *                    noise -- the caller's reason to reject a row
 *   output           phi(n) = [PHASE] ((uint64)phase0 << 32) + [FREQ] n phase_step   (mod 2^64)
 *                    out[r, n] = mul(v, mixer(top 32 bits of 0 - phi(n))),  v = u[n] under AMCX_CARRIER_GAIN, in[r, n] otherwise;
 *                    mixer: the down-converter's (ABI 11).  The product is always formed, also by 1 + 0j.
 *
 * MODES.  out_c64_dev NULL: estimate only.  AMCX_CARRIER_GIVEN: est_dev is INPUT -- nothing is estimated, order and search_bins
 * are checked and unused, a record's gain, phase0 and phase_step are applied as they are under the three apply flags (one
 * estimate for many frames of an emitter, or one smoothed on the host); out is then required.
 * POSITION INDEPENDENCE.  A record's and a row's bits depend on that row's samples and the scalar arguments alone: not on the
 * row's place in the call, the strides, the grid, or a start on 8 rather than 16 bytes.  Only phase0 goes through a library
 * routine (atan2f) and is held to a bound; every other field and, given the record, every output sample is exact.
 *
 *   - limits: n a power of two of 64 ... 4096; order 1, 2, 4 or 8; 0 <= search_bins <= n / 2 - 1; no flag but the four; GIVEN
 *     needs out; 0 <= n_rows, in_row_stride >= n, out_row_stride >= n where out is given, n_rows times either stride <= 2^58;
 *     at most 2^31 - 1 groups of 4096 / n rows
 *   - checks, in the order of every launching entry: the limits in that order; n_rows == 0 is AMCX_OK here and writes nothing;
 *     then null pointers (in, est), alignment (all 8), a pointer on another device, and the byte ranges of in and out, which
 *     must not overlap.  Ordinary vector stores only.
 * amcx_carrier_plan (host-only): the rows a workgroup holds (4096 / n) and its bytes of static LDS; each pointer may be NULL.
 * amcx_kernel_name_carrier (host-only): the kernel's name, a static string.
 */
#define AMCX_CARRIER_GAIN 1u
#define AMCX_CARRIER_FREQ 2u
#define AMCX_CARRIER_PHASE 4u
#define AMCX_CARRIER_GIVEN 8u
int amcx_carrier_plan(int32_t n, int32_t* rows_per_workgroup, int32_t* lds_bytes);
int amcx_carrier_c64(const void* in_c64_dev, int64_t n_rows, int32_t n, int64_t in_row_stride, int32_t order, int32_t search_bins,
                     uint32_t flags, void* est_dev, void* out_c64_dev, int64_t out_row_stride, void* hip_stream);
const char* amcx_kernel_name_carrier(void);

#ifdef __cplusplus
}
#endif
#endif /* AMCX_H_ */
