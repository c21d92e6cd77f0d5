"""The demultiplexing's kernels (dmx.hip) as the compiler leaves them: every one present, none with scratch, none above 128 VGPRs
(four waves a SIMD).  No GPU: the kernels are compiled to assembly and the metadata is read."""
from test_kernel_resources import kernel_metadata

KERNELS = ["k_dmx_check", "k_dmx_assignILj1E", "k_dmx_assignILj2E", "k_dmx_settle", "k_dmx_hist", "k_dmx_rank", "k_dmx_count",
           "k_dmx_pieces", "k_dmx_bounds", "k_dmx_room"]


def test_demux_kernels_use_no_scratch(tmp_path):
    meta = kernel_metadata("dmx.hip", tmp_path)
    assert len([k for k in meta if "k_dmx_" in k]) == len(KERNELS), sorted(meta)
    for want in KERNELS:
        hits = [(k, v) for k, v in meta.items() if want in k]
        assert len(hits) == 1, "kernel %s not found in dmx.hip" % want
        name, (vgprs, scratch) = hits[0]
        assert scratch == 0, "%s keeps %d bytes of scratch per lane (spills or call frames)" % (name, scratch)
        assert vgprs <= 128, "%s needs %d VGPRs: fewer than 4 waves per SIMD" % (name, vgprs)
