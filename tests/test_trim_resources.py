"""Every kernel of trim.hip keeps its registers: no scratch, and 128 VGPRs at most (four waves a SIMD).  hipcc cross-compiles for
gfx950 without a GPU, so this is checked on the CPU."""
from test_kernel_resources import kernel_metadata

KERNELS = ("k_trim_check", "k_trim_lens", "k_trim_terms", "k_trim_cut", "k_trim_pieces", "k_trim_room")


def test_the_trim_kernels_use_no_scratch(tmp_path):
    meta = kernel_metadata("trim.hip", tmp_path)
    for want in KERNELS:
        assert any(want in k for k in meta), "kernel %s not found in trim.hip" % want
    assert len([k for k in meta if "k_trim_terms" in k]) >= 15         # one per set of terms that are on
    for name, (vgprs, scratch) in meta.items():
        assert scratch == 0, "%s keeps %d bytes of scratch per lane (spills or call frames)" % (name, scratch)
        assert vgprs <= 128, "%s needs %d VGPRs: fewer than 4 waves per SIMD" % (name, vgprs)
