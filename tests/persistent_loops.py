"""Every persistent launch of the library and the GPU test that takes its grid-stride loop round three times.

A persistent launch is `persistent_grid(cus, wgs_per_cu, work, unit)` workgroups, each walking
`for (item = blockIdx.x; item < n; item += gridDim.x)`.  A test whose work fits the grid runs every loop body once and never
executes the loop's tail barrier, the re-derivation of per-item state, the tables that must survive a trip, or `item * stride`
at larger indices.  So every call site of `persistent_grid(` in amcpy_amd/csrc/amcx.hip and amcx_launch.h has ONE entry here, in
the order of the source: the file, the launch (its kernels' stem), and the tests -- (file, function) -- that give it at least
2 grid + 1 units of work, the grid read from the library's plan or restated from the call site beside the device's CU count.
Each of those tests asserts `units >= 2 * grid + 1` itself and prints both numbers.

tests/test_persistent_loops_host.py holds the table to the source: as many entries per file as the file has call sites, and
every named test exists.  A new persistent launch therefore cannot arrive without naming its test."""

SOURCES = ("amcpy_amd/csrc/amcx.hip", "amcpy_amd/csrc/amcx_launch.h")

_LOOPS = "tests/test_gpu_persistent_loops.py"
_FEATURES = (_LOOPS, "test_feature_rows_over_three_trips_of_the_grid")
_INTEGERS = (_LOOPS, "test_integer_frames_over_three_trips_of_the_grid")
_PSD, _OCC = "tests/test_gpu_psd.py", "tests/test_gpu_occupancy.py"
_SYNTH, _CHAIN = "tests/test_gpu_synth.py", "tests/test_gpu_chain_exact.py"

# (source file, the launch, ((test file, test function), ...)) in the order of the call sites in each file
TABLE = (
    ("amcpy_amd/csrc/amcx.hip", "stream_plan: amcx_features18_stream_kernel, 8192 < N <= 32768 outside the table",
     (_FEATURES, (_LOOPS, "test_stream_kernel_without_a_workspace_over_three_trips_of_the_grid"))),
    ("amcpy_amd/csrc/amcx.hip", "launch_block_mode: amcx_features18_block_kernel<0 ... 3>", (_FEATURES,)),
    ("amcpy_amd/csrc/amcx.hip", "launch_sc16_widen: amcx_sc16_to_c64_kernel", (_INTEGERS,)),
    ("amcpy_amd/csrc/amcx.hip", "launch_iq8_widen: amcx_iq8_to_sc16_kernel, amcx_iq8_to_c64_kernel", (_INTEGERS,)),
    ("amcpy_amd/csrc/amcx.hip", "down-converter kernel launch: amcx_tune_decimate_*",
     (("tests/test_gpu_ddc.py", "test_parity_over_three_trips_of_the_grid"),)),
    ("amcpy_amd/csrc/amcx.hip", "filter-bank kernel launch: amcx_filter_bank_*",
     (("tests/test_gpu_bank.py", "test_criterion_against_float64_over_three_trips_of_the_grid"),
      (_CHAIN, "test_filter_bank_transform_alone_over_three_trips_of_the_grid"),
      (_CHAIN, "test_filter_bank_exact_over_three_trips_of_the_grid"))),
    ("amcpy_amd/csrc/amcx.hip", "resampler kernel launch: amcx_resample_*",
     (("tests/test_gpu_resample.py", "test_parity_over_three_trips_of_the_grid"),)),
    ("amcpy_amd/csrc/amcx.hip", "row-power kernel launch: amcx_row_power_kernel",
     ((_OCC, "test_power_criterion_over_three_trips_of_the_grid"),)),
    ("amcpy_amd/csrc/amcx.hip", "occupancy floor kernel launch: amcx_occupancy_detect_kernel",
     ((_OCC, "test_detect_exact_over_three_trips_of_the_floor_grid"),)),
    ("amcpy_amd/csrc/amcx.hip", "occupancy count and scatter kernel launches: amcx_occupancy_{count,scatter}_kernel",
     ((_OCC, "test_detect_exact_over_three_trips_of_the_floor_grid"),)),
    ("amcpy_amd/csrc/amcx.hip", "row-gather kernel launch: amcx_gather_rows_kernel", ((_OCC, "test_gather_over_three_trips_of_the_grid"),)),
    ("amcpy_amd/csrc/amcx.hip", "spectrogram kernel launch: amcx_spectrogram_{c64,sc16,iq8}_kernel",
     ((_PSD, "test_rows_equal_the_float32_restatement_over_three_trips_of_the_grid"),
      (_PSD, "test_integer_formats_are_the_complex64_bits_over_three_trips_of_the_grid"),
      (_PSD, "test_padding_is_untouched_over_three_trips_of_the_grid"))),
    ("amcpy_amd/csrc/amcx.hip", "spectrogram detection kernel launch: amcx_psd_detect_kernel",
     ((_PSD, "test_detect_equals_numpy_over_three_trips_of_the_grid"),)),
    ("amcpy_amd/csrc/amcx.hip", "select-and-scale kernel launch: amcx_select_scale_kernel",
     ((_LOOPS, "test_select_scale_over_three_trips_of_the_grid"),)),
    ("amcpy_amd/csrc/amcx.hip", "classifier kernel launch: amcx_mlp_classify_kernel", ((_LOOPS, "test_classifier_over_three_trips_of_the_grid"),)),
    ("amcpy_amd/csrc/amcx.hip", "range kernel launch: amcx_mlp_range_kernel", ((_LOOPS, "test_ranges_over_three_trips_of_the_grid"),)),
    ("amcpy_amd/csrc/amcx.hip", "Q15 classifier kernel launch: amcx_mlp_q15_kernel", ((_LOOPS, "test_q15_over_three_trips_of_the_grid"),)),
    ("amcpy_amd/csrc/amcx.hip", "waveform generator kernel launch: amcx_synth_c64_kernel",
     ((_SYNTH, "test_every_row_over_three_trips_of_the_grid"),)),
    ("amcpy_amd/csrc/amcx_launch.h", "ShortSize: amcx_features18_short_kernel and its sc16 and plan kernels, N = 128, 256, 512",
     (_FEATURES, _INTEGERS, (_LOOPS, "test_plan_kernels_over_three_trips_of_the_grid"))),
    ("amcpy_amd/csrc/amcx_launch.h", "WaveSize: amcx_features18_wave_kernel and its sc16 and plan kernels, N = 1024, 2048, 4096",
     (_FEATURES, _INTEGERS, (_LOOPS, "test_plan_kernels_over_three_trips_of_the_grid"))),
    ("amcpy_amd/csrc/amcx_launch.h", "QuadSize: amcx_features18_quad_kernel, N = 8192", (_FEATURES,)),
    ("amcpy_amd/csrc/amcx_launch.h", "GroupSize: amcx_features18_group_kernel, N = 16384, 32768", (_FEATURES,)),
)
