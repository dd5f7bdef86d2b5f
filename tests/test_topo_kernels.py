"""CPU-only checks of the code object of icebin_amd/csrc/topo.hip: every kernel is wave64 and none uses scratch
memory, by the gfx950 code object's metadata."""
import re

from icebin_amd.build import build_library
from test_capi_symbols import code_object_notes


def test_topo_kernels_are_wave64_without_scratch(tmp_path):
    build_library()
    notes = code_object_notes(tmp_path, "topo")
    names = re.findall(r"^    \.name:\s+(\S+)", notes, re.M)
    scratch = [int(s) for s in re.findall(r"^    \.private_segment_fixed_size:\s+(\d+)", notes, re.M)]
    waves = [int(s) for s in re.findall(r"^    \.wavefront_size:\s+(\d+)", notes, re.M)]
    assert len(names) == len(scratch) == len(waves) >= 13, (len(names), len(scratch), len(waves))
    assert all("k_topo" in n for n in names), names
    assert sum("k_topo_row_stats" in n for n in names) == 2         # the 4-wave and the 16-wave workgroup
    assert not [(n, s) for n, s in zip(names, scratch) if s != 0]
    assert set(waves) == {64}
