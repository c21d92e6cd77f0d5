"""Every kernel of scr.hip keeps its registers: no scratch, and 128 VGPRs at most (four waves a SIMD).  hipcc cross-compiles for
gfx950 without a GPU, so this is checked on the CPU."""
from test_kernel_resources import kernel_metadata

KERNELS = ("k_scr_add", "k_scr_check", "k_scr_count", "k_scr_verdict", "k_scr_scatter", "k_scr_room")


def test_the_screen_kernels_use_no_scratch(tmp_path):
    meta = kernel_metadata("scr.hip", tmp_path)
    for want in KERNELS:
        assert any(want in k for k in meta), "kernel %s not found in scr.hip" % want
    assert len([k for k in meta if "k_scr_count" in k]) >= 4           # one per number of lanes a record
    assert len([k for k in meta if "k_scr_verdict" in k]) >= 2         # records, pairs
    for name, (vgprs, scratch) in meta.items():
        assert scratch == 0, "%s keeps %d bytes of scratch per lane (spills or call frames)" % (name, scratch)
        assert vgprs <= 128, "%s needs %d VGPRs: fewer than 4 waves per SIMD" % (name, vgprs)
