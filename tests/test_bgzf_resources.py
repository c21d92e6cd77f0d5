"""The BGZF pass's kernels (bgz.hip) as the compiler leaves them: every one present, none with scratch, none above 128 VGPRs.  No GPU:
the kernels are compiled to assembly and the metadata is read."""
from test_kernel_resources import kernel_metadata

KERNELS = ["k_bgz_deflate", "k_bgz_room", "k_bgz_from"]


def test_bgzf_kernels_use_no_scratch(tmp_path):
    meta = kernel_metadata("bgz.hip", tmp_path)
    assert len([k for k in meta if "k_bgz_" in k]) == len(KERNELS), sorted(meta)
    for want in KERNELS:
        hits = [(k, v) for k, v in meta.items() if want in k]
        assert len(hits) == 1, "kernel %s not found in bgz.hip" % want
        name, (vgprs, scratch) = hits[0]
        assert scratch == 0, "%s keeps %d bytes of scratch per lane (spills or call frames)" % (name, scratch)
        assert vgprs <= 128, "%s needs %d VGPRs" % (name, vgprs)
