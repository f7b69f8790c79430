"""Every plain-grid launch of the library that is folded into lines, and the GPU test that runs more than one line of it.

The three kernels that do not use `persistent_grid` launch one workgroup per item.  A call with more than LINE = 65 536 items
is folded into a 2-D grid in amcpy_amd/csrc/amcx.hip:

    gx = n < 65536 ? n : 65536,  gy = (n + gx - 1) / gx
    item = (long long)blockIdx.y * gridDim.x + blockIdx.x;   if (item >= n) return;

A test with at most LINE items never executes the `blockIdx.y` term, the whole-workgroup `return` of the grid's last line, or
`item * stride` at an item index of 2^16 or more.  So every launch with `dim3((unsigned)gx, (unsigned)gy)` in amcx.hip has ONE
entry here, in the order of the source: the launch and its kernel, and the tests -- (file, function) -- that give it at least
2 LINE + 1 items (three lines, the last with one live workgroup), each of which asserts `items >= 2 * LINE + 1` itself and
prints the count.  The carrier's workgroup always holds 4096 points, so a line of it is 2.1 GB of input whatever N: its test
stops at LINE + 1 groups, two lines, the second with one live workgroup and 65 535 that return, and asserts `>= LINE + 1`.

tests/test_plain_grids_host.py holds the table to the source: as many entries as amcx.hip has such launches, every named test
exists, and each kernel's header decodes its item as above.  A new folded launch therefore cannot arrive without naming its
test."""

LINE = 65536
SOURCE = "amcpy_amd/csrc/amcx.hip"

_CHANNEL, _CPM, _CARRIER = "tests/test_gpu_channel.py", "tests/test_gpu_cpm.py", "tests/test_gpu_carrier.py"

# (the launch and its kernel, ((test file, test function), ...)) in the order of the call sites
TABLE = (
    ("channel kernel launch: amcx_channel_c64_kernel, one workgroup per (row, tile)",
     ((_CHANNEL, "test_rows_over_three_lines_of_the_grid"),)),
    ("continuous-phase generator kernel launch: amcx_synth_cpm_c64_kernel, one workgroup per (row, segment)",
     ((_CPM, "test_rows_over_three_lines_of_the_grid"),)),
    ("carrier recovery kernel launch: amcx_carrier_c64_kernel, one workgroup per group of 4096 / N rows",
     ((_CARRIER, "test_rows_over_two_lines_of_the_grid"),)),
)

# the headers of the kernels behind the entries, in the same order: each decodes its item from both grid dimensions
HEADERS = ("amcpy_amd/csrc/amcx_channel_kernel.h", "amcpy_amd/csrc/amcx_synth_cpm_kernel.h", "amcpy_amd/csrc/amcx_carrier_kernel.h")

# the assertion a named file carries: three lines, but two for the carrier (above)
BOUND = {_CHANNEL: ">= 2 * LINE + 1", _CPM: ">= 2 * LINE + 1", _CARRIER: ">= LINE + 1"}
