"""Every kernel of sel.hip keeps its registers: no scratch, and 128 VGPRs at most (four waves a SIMD).  hipcc cross-compiles for
gfx950 without a GPU, so this is checked on the CPU."""
from test_kernel_resources import kernel_metadata

KERNELS = ("k_sel_starts", "k_sel_check", "k_sel_terms", "k_sel_verdict", "k_sel_scatter", "k_sel_room")


def test_the_selection_kernels_use_no_scratch(tmp_path):
    meta = kernel_metadata("sel.hip", tmp_path)
    for want in KERNELS:
        assert any(want in k for k in meta), "kernel %s not found in sel.hip" % want
    assert len([k for k in meta if "k_sel_terms" in k]) >= 7           # one per set of terms that are on
    for name, (vgprs, scratch) in meta.items():
        assert scratch == 0, "%s keeps %d bytes of scratch per lane (spills or call frames)" % (name, scratch)
        assert vgprs <= 128, "%s needs %d VGPRs: fewer than 4 waves per SIMD" % (name, vgprs)
