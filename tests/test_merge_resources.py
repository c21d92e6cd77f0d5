"""Every kernel of mrg.hip keeps its registers: no scratch, and 128 VGPRs at most (four waves a SIMD).  hipcc cross-compiles for
gfx950 without a GPU, so this is checked on the CPU."""
from test_kernel_resources import kernel_metadata

KERNELS = ("k_mrg_plan", "k_mrg_room", "k_mrg_list", "k_mrg_write")


def test_the_merge_kernels_use_no_scratch(tmp_path):
    meta = kernel_metadata("mrg.hip", tmp_path)
    for want in KERNELS:
        assert any(want in k for k in meta), "kernel %s not found in mrg.hip" % want
    for name, (vgprs, scratch) in meta.items():
        assert scratch == 0, "%s keeps %d bytes of scratch per lane (spills or call frames)" % (name, scratch)
        assert vgprs <= 128, "%s needs %d VGPRs: fewer than 4 waves per SIMD" % (name, vgprs)
