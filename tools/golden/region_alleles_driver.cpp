// region_alleles_driver.cpp -- records what the REFERENCE's active regions leave in the indel buffer and the candidate SNV buffer once
// their haplotypes are selected: the vectors under tests/golden/region_alleles/ that anchor tests/alleles_model.py.
//
// TEST INFRASTRUCTURE ONLY; contains no reference code, and is never needed to run the tests: it is built by hand on a machine
// that has the reference tree and the objects oracle/Makefile compiles from it (`make -C oracle ref`):
//
//   L=$REFERENCE/src/c++/lib; O=oracle/_ref
//   g++ -std=c++11 -O2 -w -ffp-contract=off -I$L -Ioracle/ref/gen -Ioracle/boost_shim -I$O/redist/htslib-1.7-6-g6d2bfb7 \
//       -I$O/redist/rapidjson-1.1.0/include -Ioracle/ref tools/golden/region_alleles_driver.cpp $O/libreftus.a \
//       $O/redist/htslib-1.7-6-g6d2bfb7/libhts.a -lm -lz -lpthread -o $O/bin/region_alleles_driver
//   python tools/golden/make_region_alleles_golden.py $O/bin/region_alleles_driver
//
// The reads go into the detector's read buffer as in region_haplotypes_driver.cpp.  Per region, with the _prevActiveRegionEnd the
// input names: ActiveRegionProcessor::processHaplotypes (ActiveRegionProcessor.cpp:45-77) -- where counting succeeds, so that the
// assembler never runs -- into an IndelBuffer and a CandidateSnvBuffer of the region's own, both read out afterwards.
//
// stdin:   REF <offset> <sequence>
//          OPT <max_indel_size>
//          BUF <begin> <end>                                      _readBufferRange
//          READ <pos> <is_low_mapq> <is_fwd_strand> <sequence> <n_seg> (<type> <length>)...      type = ALIGNPATH::align_t
//          REGION <begin> <end> <ploidy> <prev_end>
//          TIME <repeats>                                         processSelectedHaplotypes of every counted region, timed
// stdout:  one JSON document
#include <map>
#include <memory>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#define private public // (the read buffer's range, the processor's selections and the indel buffer's map are private members; first, before any header that includes these)
#include "starling_common/IndelBuffer.hh"
#include "starling_common/ActiveRegionReadBuffer.hh"
#include "starling_common/ActiveRegionProcessor.hh"
#undef private

#include "appstats/RunStatsManager.hh"
#include "options/AlignmentFileOptions.hh"
#include "starling_common/ActiveRegionDetector.hh"
#include "starling_common/CandidateSnvBuffer.hh"
#include "starling_common/starling_base_shared.hh"
#include "starling_common/starling_read_util.hh"
#include "starling_common/starling_streams_base.hh"
#include "starling_common/starling_pos_processor_base.hh"
#include "starling_common/starling_pos_processor_indel_util.hh"

#include <chrono>
#include <cstdio>
#include <cstring>
#include <iostream>

namespace
{

struct Streams : public starling_streams_base
{
    explicit Streams(const unsigned n) : starling_streams_base(n) {}
};

struct PP : public starling_pos_processor_base
{
    PP(const starling_base_options& opt, const starling_base_deriv_options& dopt, const reference_contig_segment& ref, const Streams& streams,
       RunStatsManager& stats)
        : starling_pos_processor_base(opt, dopt, ref, streams, 1, stats)
    {
        sample_info& sif(sample(0));
        getIndelBuffer().registerSample(sif.estdepth_buff, sif.estdepth_buff_tier2, true);
        getIndelBuffer().finalizeSamples();
    }
    void resetRegion(const known_pos_range2& range) { resetRegionBase("chrT", range); }
    void process_pos_variants_impl(const pos_t, const bool) override {}
};

struct DriverOptions : public starling_base_options
{
    const AlignmentFileOptions& getAlignmentFileOptions() const override
    {
        static AlignmentFileOptions alignFileOpt;
        if (alignFileOpt.alignmentFilenames.empty()) alignFileOpt.alignmentFilenames.push_back("sample.bam");
        return alignFileOpt;
    }
};

struct Read
{
    int pos, low_mapq, is_fwd;
    std::string seq;
    std::vector<std::pair<int, unsigned>> path;
};

struct Region
{
    int begin, end;
    unsigned ploidy;
    int prev_end;
};

unsigned float_bits(const float x)
{
    unsigned u;
    std::memcpy(&u, &x, sizeof(u));
    return u;
}

} // namespace

int main()
{
    std::string ref_seq;
    int ref_offset = 0, buf_begin = 0, buf_end = 0, time_repeats = 0;
    unsigned max_indel_size = 49;
    std::vector<Read> reads;
    std::vector<Region> regions;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        std::string tag;
        is >> tag;
        if (tag == "REF") is >> ref_offset >> ref_seq;
        else if (tag == "OPT") is >> max_indel_size;
        else if (tag == "BUF") is >> buf_begin >> buf_end;
        else if (tag == "TIME") is >> time_repeats;
        else if (tag == "REGION") {
            Region g;
            is >> g.begin >> g.end >> g.ploidy >> g.prev_end;
            regions.push_back(g);
        } else if (tag == "READ") {
            Read r;
            int n_seg = 0;
            is >> r.pos >> r.low_mapq >> r.is_fwd >> r.seq >> n_seg;
            for (int i = 0; i < n_seg; ++i) {
                int t;
                unsigned l;
                is >> t >> l;
                r.path.push_back(std::make_pair(t, l));
            }
            reads.push_back(r);
        }
    }
    try {
        DriverOptions opt;
        opt.isHaplotypingEnabled = true;
        opt.maxIndelSize = max_indel_size;
        starling_base_deriv_options dopt(opt);
        reference_contig_segment ref;
        ref.seq() = ref_seq;
        ref.set_offset(ref_offset);
        Streams streams(1);
        RunStatsManager stats("");
        PP pp(opt, dopt, ref, streams, stats);
        pp.resetRegion(known_pos_range2(0, 1000));
        const std::pair<bool, bool> no_pin(false, false);
        for (size_t i = 0; i < reads.size(); ++i) {
            const Read& r(reads[i]);
            bam_record br;
            alignment al;
            const std::vector<uint8_t> qual(r.seq.size(), 30);
            br.set_qname("R");
            br.set_readqual(r.seq.c_str(), qual.data());
            al.pos = r.pos;
            al.is_fwd_strand = r.is_fwd != 0;
            for (const auto& s : r.path) al.path.push_back(ALIGNPATH::path_segment(static_cast<ALIGNPATH::align_t>(s.first), s.second));
            const bam_seq bseq(br.get_bam_read());
            addAlignmentIndelsToPosProcessor(max_indel_size, ref, al, bseq, pp, INDEL_ALIGN_TYPE::GENOME_TIER1_READ, static_cast<align_id_t>(i), 0, no_pin,
                                             r.low_mapq != 0);
        }
        ActiveRegionReadBuffer& rb(pp.getActiveRegionReadBuffer(0));
        rb._readBufferRange.set_begin_pos(buf_begin);
        rb._readBufferRange.set_end_pos(buf_end);
        const GlobalAligner<int> aligner(AlignmentScores<int>(ActiveRegionDetector::ScoreMatch, ActiveRegionDetector::ScoreMismatch, ActiveRegionDetector::ScoreOpen,
                                                              ActiveRegionDetector::ScoreExtend, ActiveRegionDetector::ScoreOffEdge, ActiveRegionDetector::ScoreOpen,
                                                              true, true));
        // does counting succeed (generateHaplotypesWithCounting :79-93)?  Otherwise processHaplotypes would go on to the assembler.
        auto is_counted = [&](const Region& g, const ActiveRegionReadInfo& info) {
            const known_pos_range2 range(g.begin, g.end);
            const bool in_range(g.begin >= buf_begin && g.end <= buf_end && range.size() <= ActiveRegionProcessor::MaxRefSpanToBypassAssembly);
            return in_range && info.numReadsAlignedToActiveRegion != 0 &&
                   !(info.readSegmentsForHaplotypeGeneration.size() < (0.65f * info.numReadsAlignedToActiveRegion));
        };

        if (time_repeats > 0) { // processSelectedHaplotypes of every counted region, on this core; the selection and the buffers are made outside the clock
            double seconds = 0;
            size_t sink = 0, n_counted = 0;
            for (int rep = 0; rep < time_repeats; ++rep) {
                for (const Region& g : regions) {
                    const known_pos_range2 range(g.begin, g.end);
                    ActiveRegionReadInfo info;
                    rb.getReadSegments(range, info, false);
                    if (!is_counted(g, info)) continue;
                    IndelBuffer regionBuffer(opt, dopt, ref);
                    depth_buffer db, db2;
                    regionBuffer.registerSample(db, db2, false);
                    regionBuffer.finalizeSamples();
                    CandidateSnvBuffer regionSnvBuffer(1);
                    ActiveRegionProcessor arp(range, g.prev_end, ref, max_indel_size, 0, g.ploidy, aligner, rb, regionBuffer, regionSnvBuffer);
                    arp._numReadsUsedToGenerateHaplotypes = info.numReadsAlignedToActiveRegion;
                    HaplotypeToAlignIdSet sets;
                    for (const auto& entry : info.readSegmentsForHaplotypeGeneration) sets[entry.second].push_back(entry.first);
                    arp.selectHaplotypes(sets);
                    const auto t0(std::chrono::steady_clock::now());
                    arp.processSelectedHaplotypes();
                    seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
                    sink += regionBuffer._indelBuffer.size();
                    if (rep == 0) ++n_counted;
                }
            }
            std::printf("{\"time_repeats\": %d, \"regions\": %zu, \"counted\": %zu, \"seconds_per_pass\": %.9f, \"keys\": %zu}\n", time_repeats, regions.size(), n_counted,
                        seconds / time_repeats, sink);
            return 0;
        }

        std::printf("{\"ref_offset\": %d, \"ref\": \"%s\", \"max_indel_size\": %u, \"buf_begin\": %d, \"buf_end\": %d, \"reads\": [\n", ref_offset, ref_seq.c_str(),
                    max_indel_size, buf_begin, buf_end);
        for (size_t i = 0; i < reads.size(); ++i) {
            const Read& r(reads[i]);
            std::printf("{\"pos\": %d, \"low_mapq\": %d, \"is_fwd\": %d, \"seq\": \"%s\", \"path\": [", r.pos, r.low_mapq, r.is_fwd, r.seq.c_str());
            for (size_t k = 0; k < r.path.size(); ++k) std::printf("%s[%d, %u]", k ? ", " : "", r.path[k].first, r.path[k].second);
            std::printf("]}%s\n", i + 1 < reads.size() ? "," : "");
        }
        std::printf("], \"regions\": [\n");
        for (size_t gi = 0; gi < regions.size(); ++gi) {
            const Region& g(regions[gi]);
            const known_pos_range2 range(g.begin, g.end);
            ActiveRegionReadInfo info;
            rb.getReadSegments(range, info, false);
            std::printf("{\"begin\": %d, \"end\": %d, \"ploidy\": %u, \"prev_end\": %d, \"n_reads_aligned\": %u", g.begin, g.end, g.ploidy, g.prev_end,
                        info.numReadsAlignedToActiveRegion);
            IndelBuffer regionBuffer(opt, dopt, ref);
            depth_buffer db, db2;
            regionBuffer.registerSample(db, db2, false);
            regionBuffer.finalizeSamples();
            CandidateSnvBuffer regionSnvBuffer(1);
            ActiveRegionProcessor arp(range, g.prev_end, ref, max_indel_size, 0, g.ploidy, aligner, rb, regionBuffer, regionSnvBuffer);
            const bool counted(is_counted(g, info));
            std::printf(", \"counted\": %d, \"selected\": [", counted ? 1 : 0);
            if (counted) {
                arp.processHaplotypes();
                for (size_t k = 0; k < arp._selectedHaplotypes.size(); ++k) {
                    std::printf("%s{\"seq\": \"%s\", \"support\": [", k ? ", " : "", arp._selectedHaplotypes[k].c_str());
                    for (size_t j = 0; j < arp._selectedAlignIdLists[k].size(); ++j) std::printf("%s%u", j ? ", " : "", unsigned(arp._selectedAlignIdLists[k][j]));
                    std::printf("]}");
                }
            }
            // every key of the indel buffer, in its order (IndelKey::operator<)
            std::printf("], \"keys\": [");
            bool first(true);
            for (const auto& entry : regionBuffer._indelBuffer) {
                const IndelKey& key(entry.first);
                const IndelData& data(entry.second);
                const IndelSampleData& sd(data.getSampleData(0));
                std::printf("%s{\"pos\": %d, \"type\": %d, \"del_len\": %u, \"ins\": \"%s\", \"active_region_id\": %d, \"haplotype_id\": %u, \"ratio\": %u, \"ids\": [", first ? "" : ", ",
                            int(key.pos), int(key.type), unsigned(key.deletionLength), key.insertSequence.c_str(), int(data.activeRegionId), unsigned(sd.haplotypeId),
                            float_bits(sd.altAlleleHaplotypeCountRatio));
                bool first_id(true);
                for (const auto id : sd.tier1_map_read_ids) {
                    std::printf("%s%u", first_id ? "" : ", ", unsigned(id));
                    first_id = false;
                }
                std::printf("]}");
                first = false;
            }
            // the candidate SNV buffer: per position the haplotype ids of A, C, G, T and the ratio
            std::printf("], \"snvs\": [");
            first = true;
            for (int pos = g.begin - 8; pos < g.end + 1300; ++pos) {
                unsigned ids[4];
                bool any(false);
                for (int b = 0; b < 4; ++b) {
                    ids[b] = regionSnvBuffer.getHaplotypeId(0, pos, static_cast<BASE_ID::index_t>(b));
                    any = any || ids[b] != 0;
                }
                if (!any) continue;
                std::printf("%s[%d, %u, %u, %u, %u, %u]", first ? "" : ", ", pos, ids[0], ids[1], ids[2], ids[3], float_bits(regionSnvBuffer.getAltHaplotypeCountRatio(0, pos)));
                first = false;
            }
            std::printf("]}%s\n", gi + 1 < regions.size() ? "," : "");
        }
        std::printf("]}\n");
    } catch (const std::exception& e) {
        std::fprintf(stderr, "region_alleles_driver: %s\n", e.what());
        return 1;
    } catch (...) {
        std::fprintf(stderr, "region_alleles_driver: exception\n");
        return 1;
    }
    return 0;
}
