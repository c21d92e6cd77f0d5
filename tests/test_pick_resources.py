"""pick.hip's kernels (picked lines) must not use scratch memory and must leave room for four waves per SIMD.
hipcc cross-compiles for gfx950 without a GPU, so this is checked on the CPU."""
from test_kernel_resources import kernel_metadata

KERNELS = ("k_pick_starts", "k_pick_check", "k_pick_lens", "k_pick_room", "k_pick_copy")


def test_pick_kernels_use_no_scratch_and_at_most_128_vgprs(tmp_path):
    meta = kernel_metadata("pick.hip", tmp_path)
    assert meta, "no kernel found in pick.hip"
    for want in KERNELS:
        assert any(want in k for k in meta), "kernel %s not found in pick.hip" % want
    for name, (vgprs, scratch) in meta.items():                      # every kernel of the file
        assert scratch == 0, "%s keeps %d bytes of scratch per lane (spills or call frames)" % (name, scratch)
        assert vgprs <= 128, "%s needs %d VGPRs: fewer than 4 waves per SIMD" % (name, vgprs)
