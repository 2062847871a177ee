// region_haplotypes_driver.cpp -- records what the REFERENCE keeps per read for haplotype generation and what it selects: the vectors
// under tests/golden/region_haplotypes/ that anchor tests/haplotype_model.py.
//
// TEST INFRASTRUCTURE ONLY; contains no reference code, and is never needed to run the tests: it is built by hand on a machine
// that has the reference tree and the objects oracle/Makefile compiles from it (`make -C oracle ref`):
//
//   L=$REFERENCE/src/c++/lib; O=oracle/_ref
//   g++ -std=c++11 -O2 -w -ffp-contract=off -I$L -Ioracle/ref/gen -Ioracle/boost_shim -I$O/redist/htslib-1.7-6-g6d2bfb7 \
//       -I$O/redist/rapidjson-1.1.0/include -Ioracle/ref tools/golden/region_haplotypes_driver.cpp $O/libreftus.a \
//       $O/redist/htslib-1.7-6-g6d2bfb7/libhts.a -lm -lz -lpthread -o $O/bin/region_haplotypes_driver
//   python tools/golden/make_region_haplotypes_golden.py $O/bin/region_haplotypes_driver
//
// The reads go through the reference's own addAlignmentIndelsToPosProcessor (L/starling_common/starling_pos_processor_indel_util.cpp:
// 300-491) into the detector's read buffer, read by read in input order (a read's index is its align id); the head position is never
// advanced, so nothing clears the buffer (the caller keeps every position inside [0, 1000) and the read count below 1 000).  Per
// region: ActiveRegionReadBuffer::getReadSegments (ActiveRegionReadBuffer.cpp:191-256) as generateHaplotypesWithCounting calls it, and
// -- where counting succeeds, so that the assembler never runs -- ActiveRegionProcessor::processHaplotypes
// (ActiveRegionProcessor.cpp:45-77) with its _selectedHaplotypes and _selectedAlignIdLists read out afterwards.
//
// stdin:   REF <offset> <sequence>
//          OPT <max_indel_size>
//          BUF <begin> <end>                                      _readBufferRange
//          READ <pos> <is_low_mapq> <is_fwd_strand> <sequence> <n_seg> (<type> <length>)...      type = ALIGNPATH::align_t
//          REGION <begin> <end> <ploidy>
//          TIME <repeats>                                         getReadSegments + counting + selection of every region, timed
// stdout:  one JSON document
#include <map>
#include <memory>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#define private public // (the read buffer's range and the processor's selections are private members; first, before any header that includes these)
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
    IndelBuffer& indels() { return getIndelBuffer(); }
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
};

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
            is >> g.begin >> g.end >> g.ploidy;
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
        CandidateSnvBuffer snvBuffer(1);
        const GlobalAligner<int> aligner(AlignmentScores<int>(ActiveRegionDetector::ScoreMatch, ActiveRegionDetector::ScoreMismatch, ActiveRegionDetector::ScoreOpen,
                                                              ActiveRegionDetector::ScoreExtend, ActiveRegionDetector::ScoreOffEdge, ActiveRegionDetector::ScoreOpen,
                                                              true, true));

        if (time_repeats > 0) { // getReadSegments + generateHaplotypesWithCounting's grouping + selectHaplotypes of every region, on this core
            size_t sink = 0;
            IndelBuffer timedBuffer(opt, dopt, ref); // (selectHaplotypes does not touch it)
            const auto t0(std::chrono::steady_clock::now());
            for (int rep = 0; rep < time_repeats; ++rep) {
                for (const Region& g : regions) {
                    const known_pos_range2 range(g.begin, g.end);
                    if (g.begin < buf_begin || g.end > buf_end || range.size() > ActiveRegionProcessor::MaxRefSpanToBypassAssembly) continue;
                    ActiveRegionProcessor arp(range, g.begin, ref, max_indel_size, 0, g.ploidy, aligner, rb, timedBuffer, snvBuffer);
                    ActiveRegionReadInfo info;
                    rb.getReadSegments(range, info, false);
                    if (info.numReadsAlignedToActiveRegion == 0) continue;
                    if (info.readSegmentsForHaplotypeGeneration.size() < (arp.MinFracReadsCoveringRegion * info.numReadsAlignedToActiveRegion)) continue;
                    HaplotypeToAlignIdSet sets;
                    for (const auto& entry : info.readSegmentsForHaplotypeGeneration) sets[entry.second].push_back(entry.first);
                    arp.selectHaplotypes(sets);
                    sink += arp._selectedHaplotypes.size();
                }
            }
            const double s(std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
            std::printf("{\"time_repeats\": %d, \"regions\": %zu, \"seconds_per_pass\": %.9f, \"selected\": %zu}\n", time_repeats, regions.size(), s / time_repeats, sink);
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
            std::printf("{\"begin\": %d, \"end\": %d, \"ploidy\": %u, \"n_reads_aligned\": %u, \"segments\": [", g.begin, g.end, g.ploidy, info.numReadsAlignedToActiveRegion);
            for (size_t k = 0; k < info.readSegmentsForHaplotypeGeneration.size(); ++k)
                std::printf("%s[%u, \"%s\"]", k ? ", " : "", unsigned(info.readSegmentsForHaplotypeGeneration[k].first), info.readSegmentsForHaplotypeGeneration[k].second.c_str());
            // what processSelectedHaplotypes adds goes to a buffer of this region's own: regions may overlap, and are recorded at both ploidies
            IndelBuffer regionBuffer(opt, dopt, ref);
            depth_buffer db, db2;
            regionBuffer.registerSample(db, db2, false);
            regionBuffer.finalizeSamples();
            CandidateSnvBuffer regionSnvBuffer(1);
            ActiveRegionProcessor arp(range, g.begin, ref, max_indel_size, 0, g.ploidy, aligner, rb, regionBuffer, regionSnvBuffer);
            const bool in_range(g.begin >= buf_begin && g.end <= buf_end && range.size() <= ActiveRegionProcessor::MaxRefSpanToBypassAssembly);
            const bool counted(in_range && info.numReadsAlignedToActiveRegion != 0 &&
                               !(info.readSegmentsForHaplotypeGeneration.size() < (arp.MinFracReadsCoveringRegion * info.numReadsAlignedToActiveRegion)));
            std::printf("], \"counted\": %d, \"selected\": [", counted ? 1 : 0);
            if (counted) {
                arp.processHaplotypes();
                for (size_t k = 0; k < arp._selectedHaplotypes.size(); ++k) {
                    std::printf("%s{\"seq\": \"%s\", \"support\": [", k ? ", " : "", arp._selectedHaplotypes[k].c_str());
                    for (size_t j = 0; j < arp._selectedAlignIdLists[k].size(); ++j) std::printf("%s%u", j ? ", " : "", unsigned(arp._selectedAlignIdLists[k][j]));
                    std::printf("]}");
                }
            }
            std::printf("]}%s\n", gi + 1 < regions.size() ? "," : "");
        }
        std::printf("]}\n");
    } catch (const std::exception& e) {
        std::fprintf(stderr, "region_haplotypes_driver: %s\n", e.what());
        return 1;
    } catch (...) {
        std::fprintf(stderr, "region_haplotypes_driver: exception\n");
        return 1;
    }
    return 0;
}
