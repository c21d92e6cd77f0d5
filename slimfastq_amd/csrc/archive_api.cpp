// archive_api.cpp -- the ".sfq" container behind the C ABI, for hosts that assemble an archive themselves
// (the writer rank of a multi-GPU job, a binding in another language).  Host only.
#include <cstring>
#include <string>
#include <vector>

#include "container.h"

extern "C" {

int sfq_archive_write(const char* path, const char* info_text, uint32_t n_streams,
                      const char* const* names, const uint8_t* const* data, const uint64_t* sizes) {
    if (!path || !info_text || (n_streams && (!names || !data || !sizes))) return SFQ_E_ARG;
    sfqc::Archive a;
    for (const char* p = info_text; *p;) {                         // "key=value\n" lines (config.cpp:334-347)
        const char* nl = strchr(p, '\n');
        const size_t len = nl ? (size_t)(nl - p) : strlen(p);
        const char* eq = (const char*)memchr(p, '=', len);
        if (eq) a.set(std::string(p, eq), std::string(eq + 1, p + len));
        p += len + (nl ? 1 : 0);
    }
    for (uint32_t s = 0; s < n_streams; s++) {
        if (!names[s] || strlen(names[s]) > 8 || (sizes[s] && !data[s])) return SFQ_E_ARG;     // directory names are 8 bytes (filer.cpp:42-47)
        a.add(names[s], std::vector<uint8_t>(data[s], data[s] + sizes[s]));
    }
    std::string err;
    return sfqc::write_file(path, a, err) ? SFQ_OK : SFQ_E_ARG;
}

int64_t sfq_pack_block_index(const sfq_block_info* blocks, uint32_t n, uint8_t* out, uint64_t cap) {
    if (n && !blocks) return SFQ_E_ARG;
    const std::vector<uint8_t> v = sfqc::pack_block_index(std::vector<sfq_block_info>(blocks, blocks + n));
    if (!out) return (int64_t)v.size();
    if (v.size() > cap) return SFQ_E_OVERFLOW;
    memcpy(out, v.data(), v.size());
    return (int64_t)v.size();
}

void sfq_text_stats_merge(sfq_text_stats* into, const sfq_text_stats* add) {
    if (into && add) sfqc::merge_text_stats(*into, *add);
}
int64_t sfq_pack_text_stats(const sfq_text_stats* stats, uint8_t* out, uint64_t cap) {
    if (!stats) return SFQ_E_ARG;
    const std::vector<uint8_t> v = sfqc::pack_text_stats(*stats);
    if (!out) return (int64_t)v.size();
    if (v.size() > cap) return SFQ_E_OVERFLOW;
    memcpy(out, v.data(), v.size());
    return (int64_t)v.size();
}
int sfq_unpack_text_stats(const uint8_t* bytes, uint64_t n, sfq_text_stats* out) {
    if (!out || (n && !bytes)) return SFQ_E_ARG;
    return sfqc::unpack_text_stats(std::vector<uint8_t>(bytes, bytes + n), *out) ? SFQ_OK : SFQ_E_CORRUPT;
}

// Quality binning: the preset tables and the check of a caller's table (the pass itself: qmap.hip).  Phred+33.
int sfq_quality_map_preset(int preset, uint8_t lut[256]) {
    struct Bin { int lo, hi, to; };
    static const Bin illumina8[] = { {2, 9, 6}, {10, 19, 15}, {20, 24, 22}, {25, 29, 27}, {30, 34, 33}, {35, 39, 37}, {40, 93, 40} };
    static const Bin novaseq4[] = { {2, 2, 2}, {3, 14, 12}, {15, 29, 23}, {30, 93, 37} };      // synth.cpp kind 2 writes these four
    if (!lut) return SFQ_E_ARG;
    const Bin* bins; size_t n;
    if (preset == SFQ_QMAP_ILLUMINA8) { bins = illumina8; n = sizeof illumina8 / sizeof *illumina8; }
    else if (preset == SFQ_QMAP_NOVASEQ4) { bins = novaseq4; n = sizeof novaseq4 / sizeof *novaseq4; }
    else return SFQ_E_ARG;
    for (int b = 0; b < 256; b++) lut[b] = (uint8_t)b;         // Q0 and Q1 among them: "no call", and the '!' of an N (gens.cpp)
    for (size_t i = 0; i < n; i++)
        for (int q = bins[i].lo; q <= bins[i].hi; q++) lut[33 + q] = (uint8_t)(33 + bins[i].to);
    return SFQ_OK;
}
int sfq_quality_map_check(const uint8_t lut[256]) {
    if (!lut) return SFQ_E_ARG;
    for (int b = 0; b < 256; b++) {
        if (b < 33 || b > 126) { if (lut[b] != b) return SFQ_E_ARG; }
        else if (lut[b] < 33 || lut[b] > 126) return SFQ_E_ARG;
    }
    return SFQ_OK;
}

int sfq_archive_write_segments(const char* path, const char* orig_name, int level, uint32_t tables, int shared_prior,
                               uint32_t n, const sfq_segment* segs) {
    if (!path || !orig_name || (n && !segs) || (tables != SFQ_TABLES_FROZEN && tables != SFQ_TABLES_ADAPTIVE)) return SFQ_E_ARG;
    sfqc::SegmentedIndex idx;
    std::vector<uint8_t> streams[SFQ_NSTREAMS];
    for (uint32_t i = 0; i < n; i++) {
        const sfq_segment& g = segs[i];
        if (!g.n_blocks) continue;
        if (!g.blocks) return SFQ_E_ARG;
        for (int s = 0; s < SFQ_NSTREAMS; s++) {
            uint64_t want = 0;
            for (uint32_t b = 0; b < g.n_blocks; b++) want += g.blocks[b].size[s];
            if (g.stream_bytes[s] != want || (want && !g.streams[s])) return SFQ_E_ARG;
            streams[s].insert(streams[s].end(), g.streams[s], g.streams[s] + want);
        }
        idx.add(g);
    }
    if (idx.segs.empty()) return SFQ_E_ARG;                 // (an archive of no blocks does not decode)
    const bool frozen = tables == SFQ_TABLES_FROZEN;
    sfqc::Archive a;
    a.info = idx.info(level, orig_name, frozen, shared_prior != 0);
    for (int s = 0; s < SFQ_NSTREAMS; s++) if (!streams[s].empty()) a.add(sfq_stream_name(s), std::move(streams[s]));
    for (auto& s : idx.streams(frozen)) a.add(s.first, std::move(s.second));
    std::string err;
    return sfqc::write_file(path, a, err) ? SFQ_OK : SFQ_E_ARG;
}

}  // extern "C"
