"""Every kernel of ovl.hip keeps its registers: no scratch, and 128 VGPRs at most (four waves a SIMD).  hipcc cross-compiles for
gfx950 without a GPU, so this is checked on the CPU."""
from test_kernel_resources import kernel_metadata

KERNELS = ("k_ovl_check", "k_ovl_lens", "k_ovl_bad", "k_ovl_search", "k_ovl_cut", "k_ovl_pieces", "k_ovl_room")


def test_the_overlap_kernels_use_no_scratch(tmp_path):
    meta = kernel_metadata("ovl.hip", tmp_path)
    for want in KERNELS:
        assert any(want in k for k in meta), "kernel %s not found in ovl.hip" % want
    for name, (vgprs, scratch) in meta.items():
        assert scratch == 0, "%s keeps %d bytes of scratch per lane (spills or call frames)" % (name, scratch)
        assert vgprs <= 128, "%s needs %d VGPRs: fewer than 4 waves per SIMD" % (name, vgprs)
