// indel_buffer_driver.cpp -- records what the REFERENCE's IndelBuffer holds after a call's reads have been added and its active regions
// closed in order: the vectors under tests/golden/indel_table/ that anchor tests/indel_table_model.py.
//
// TEST INFRASTRUCTURE ONLY; contains no reference code, and is never needed to run the tests: it is built by hand on a machine
// that has the reference tree and the objects oracle/Makefile compiles from it (`make -C oracle ref`):
//
//   L=$REFERENCE/src/c++/lib; O=oracle/_ref
//   g++ -std=c++11 -O2 -w -ffp-contract=off -I$L -Ioracle/ref/gen -Ioracle/boost_shim -I$O/redist/htslib-1.7-6-g6d2bfb7 \
//       -I$O/redist/rapidjson-1.1.0/include -Ioracle/ref tools/golden/indel_buffer_driver.cpp $O/libreftus.a \
//       $O/redist/htslib-1.7-6-g6d2bfb7/libhts.a -lm -lz -lpthread -o $O/bin/indel_buffer_driver
//   python tools/golden/make_indel_table_golden.py $O/bin/indel_buffer_driver
//
// ONE IndelBuffer registered for S samples.  The reads go in through addAlignmentIndelsToPosProcessor with the ids and the
// INDEL_ALIGN_TYPE the scene names; then, region by region and inside a region sample by sample (closeActiveRegion's order,
// ActiveRegionDetector.cpp:204-250), ActiveRegionProcessor::processHaplotypes (ActiveRegionProcessor.cpp:45-77); then the whole map is
// written out.  Whether processHaplotypes would go on to the assembler is recomputed from the read buffer before each call
// (generateHaplotypesWithCounting's two tests, :79-93) and counted in "assembled": the make script refuses a scene where it is not 0.
//
// stdin:   REF <offset> <sequence>
//          OPT <max_indel_size>
//          SAMPLES <S>
//          BUF <sample> <begin> <end>                             _readBufferRange of the sample's read buffer
//          READ <sample> <align id> <iat> <pos> <is_low_mapq> <is_fwd_strand> <sequence> <n_seg> (<type> <length>)...
//          REGION <begin> <end> <prev_end> <ploidy of sample 0> ... <ploidy of sample S - 1>
//          TIME <repeats>                                         the whole of it -- reads, regions -- timed, the objects made outside the clock
// stdout:  one JSON document
#include <map>
#include <memory>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#define private public // (the read buffer's range and the indel buffer's map are private members; first, before any header that includes these)
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
       const unsigned n_samples, RunStatsManager& stats)
        : starling_pos_processor_base(opt, dopt, ref, streams, n_samples, stats)
    {
        for (unsigned s = 0; s < n_samples; ++s) {
            sample_info& sif(sample(s));
            getIndelBuffer().registerSample(sif.estdepth_buff, sif.estdepth_buff_tier2, true);
        }
        getIndelBuffer().finalizeSamples();
    }
    void resetRegion(const known_pos_range2& range) { resetRegionBase("chrT", range); }
    IndelBuffer& indelBuffer() { return getIndelBuffer(); }
    CandidateSnvBuffer& candidateSnvBuffer() { return getCandidateSnvBuffer(); }
    void process_pos_variants_impl(const pos_t, const bool) override {}
};

struct DriverOptions : public starling_base_options
{
    unsigned n_samples = 1;
    const AlignmentFileOptions& getAlignmentFileOptions() const override
    {
        static AlignmentFileOptions alignFileOpt;
        while (alignFileOpt.alignmentFilenames.size() < n_samples) alignFileOpt.alignmentFilenames.push_back("sample" + std::to_string(alignFileOpt.alignmentFilenames.size()) + ".bam");
        return alignFileOpt;
    }
};

struct Read
{
    int sample, id, iat, pos, low_mapq, is_fwd;
    std::string seq;
    std::vector<std::pair<int, unsigned>> path;
};

struct Region
{
    int begin, end, prev_end;
    std::vector<unsigned> ploidy;
};

unsigned float_bits(const float x)
{
    unsigned u;
    std::memcpy(&u, &x, sizeof(u));
    return u;
}

void print_ids(const char* name, const IndelSampleData::evidence_t& ids)
{
    std::printf("\"%s\": [", name);
    bool first(true);
    for (const auto id : ids) {
        std::printf("%s%u", first ? "" : ", ", unsigned(id));
        first = false;
    }
    std::printf("]");
}

} // namespace

int main()
{
    std::string ref_seq;
    int ref_offset = 0, time_repeats = 0;
    unsigned max_indel_size = 49, n_samples = 1;
    std::vector<std::pair<int, int>> buf(8, std::make_pair(0, 0));
    std::vector<Read> reads;
    std::vector<Region> regions;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        std::string tag;
        is >> tag;
        if (tag == "REF") is >> ref_offset >> ref_seq;
        else if (tag == "OPT") is >> max_indel_size;
        else if (tag == "SAMPLES") is >> n_samples;
        else if (tag == "TIME") is >> time_repeats;
        else if (tag == "BUF") {
            unsigned s;
            int b, e;
            is >> s >> b >> e;
            buf.at(s) = std::make_pair(b, e);
        } else if (tag == "REGION") {
            Region g;
            is >> g.begin >> g.end >> g.prev_end;
            for (unsigned s = 0; s < n_samples; ++s) {
                unsigned p;
                is >> p;
                g.ploidy.push_back(p);
            }
            regions.push_back(g);
        } else if (tag == "READ") {
            Read r;
            int n_seg = 0;
            is >> r.sample >> r.id >> r.iat >> r.pos >> r.low_mapq >> r.is_fwd >> r.seq >> n_seg;
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
        opt.n_samples = n_samples;
        opt.isHaplotypingEnabled = true;
        opt.maxIndelSize = max_indel_size;
        starling_base_deriv_options dopt(opt);
        reference_contig_segment ref;
        ref.seq() = ref_seq;
        ref.set_offset(ref_offset);
        Streams streams(n_samples);
        const std::pair<bool, bool> no_pin(false, false);
        const GlobalAligner<int> aligner(AlignmentScores<int>(ActiveRegionDetector::ScoreMatch, ActiveRegionDetector::ScoreMismatch, ActiveRegionDetector::ScoreOpen,
                                                              ActiveRegionDetector::ScoreExtend, ActiveRegionDetector::ScoreOffEdge, ActiveRegionDetector::ScoreOpen,
                                                              true, true));
        unsigned n_assembled = 0;
        // the whole of a call on a fresh position processor -> the processor, for the map to be read out of
        auto run = [&](double* seconds) {
            RunStatsManager* stats(new RunStatsManager("")); // (kept: the processor refers to it)
            std::unique_ptr<PP> pp(new PP(opt, dopt, ref, streams, n_samples, *stats));
            pp->resetRegion(known_pos_range2(0, 1000));
            std::vector<bam_record> records(reads.size());
            for (size_t i = 0; i < reads.size(); ++i) {
                const std::vector<uint8_t> qual(reads[i].seq.size(), 30);
                records[i].set_qname("R");
                records[i].set_readqual(reads[i].seq.c_str(), qual.data());
            }
            const auto t0(std::chrono::steady_clock::now());
            for (size_t i = 0; i < reads.size(); ++i) {
                const Read& r(reads[i]);
                alignment al;
                al.pos = r.pos;
                al.is_fwd_strand = r.is_fwd != 0;
                for (const auto& s : r.path) al.path.push_back(ALIGNPATH::path_segment(static_cast<ALIGNPATH::align_t>(s.first), s.second));
                const bam_seq bseq(records[i].get_bam_read());
                addAlignmentIndelsToPosProcessor(max_indel_size, ref, al, bseq, *pp, static_cast<INDEL_ALIGN_TYPE::index_t>(r.iat), static_cast<align_id_t>(r.id),
                                                 unsigned(r.sample), no_pin, r.low_mapq != 0);
            }
            for (unsigned s = 0; s < n_samples; ++s) {
                ActiveRegionReadBuffer& rb(pp->getActiveRegionReadBuffer(s));
                rb._readBufferRange.set_begin_pos(buf[s].first);
                rb._readBufferRange.set_end_pos(buf[s].second);
            }
            n_assembled = 0;
            for (const Region& g : regions) {
                const known_pos_range2 range(g.begin, g.end);
                for (unsigned s = 0; s < n_samples; ++s) {
                    ActiveRegionReadBuffer& rb(pp->getActiveRegionReadBuffer(s));
                    // processHaplotypes' branch conditions, recomputed: would it go on to generateHaplotypesWithAssembly?
                    const bool in_range(g.begin >= buf[s].first && g.end <= buf[s].second && range.size() <= ActiveRegionProcessor::MaxRefSpanToBypassAssembly);
                    if (in_range) {
                        ActiveRegionReadInfo info;
                        rb.getReadSegments(range, info, false);
                        if (info.numReadsAlignedToActiveRegion == 0 || info.readSegmentsForHaplotypeGeneration.size() < (0.65f * info.numReadsAlignedToActiveRegion)) ++n_assembled;
                    }
                    ActiveRegionProcessor arp(range, g.prev_end, ref, max_indel_size, s, g.ploidy[s], aligner, rb, pp->indelBuffer(), pp->candidateSnvBuffer());
                    arp.processHaplotypes();
                }
            }
            if (seconds) *seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            return pp;
        };

        if (time_repeats > 0) {
            double seconds = 0;
            size_t sink = 0;
            for (int rep = 0; rep < time_repeats; ++rep) sink += run(&seconds)->indelBuffer()._indelBuffer.size();
            std::printf("{\"time_repeats\": %d, \"reads\": %zu, \"regions\": %zu, \"samples\": %u, \"seconds_per_pass\": %.9f, \"keys\": %zu}\n", time_repeats, reads.size(),
                        regions.size(), n_samples, seconds / time_repeats, sink / time_repeats);
            return 0;
        }

        std::unique_ptr<PP> pp(run(nullptr));
        std::printf("{\"assembled\": %u, \"keys\": [\n", n_assembled);
        bool first(true);
        for (const auto& entry : pp->indelBuffer()._indelBuffer) { // in the map's order (IndelKey::operator<)
            const IndelKey& key(entry.first);
            const IndelData& data(entry.second);
            const AlleleReportInfo& info(data.getReportInfo());
            std::printf("%s{\"pos\": %d, \"type\": %d, \"del_len\": %u, \"ins\": \"%s\", \"active_region_id\": %d, \"do_not_genotype\": %d, \"it\": %d, "
                        "\"repeat_unit_len\": %u, \"ref_repeat_count\": %u, \"indel_repeat_count\": %u, \"interrupted_hpol_len\": %u, \"samples\": [",
                        first ? "" : ",\n", int(key.pos), int(key.type), unsigned(key.deletionLength), key.insertSequence.c_str(), int(data.activeRegionId),
                        data.doNotGenotype ? 1 : 0, int(info.it), unsigned(info.repeatUnitLength), unsigned(info.refRepeatCount), unsigned(info.indelRepeatCount),
                        unsigned(info.interruptedHomopolymerLength));
            for (unsigned s = 0; s < n_samples; ++s) {
                const IndelSampleData& sd(data.getSampleData(s));
                std::printf("%s{", s ? ", " : "");
                print_ids("tier1", sd.tier1_map_read_ids);
                std::printf(", ");
                print_ids("tier2", sd.tier2_map_read_ids);
                std::printf(", ");
                print_ids("submap", sd.submap_read_ids);
                std::printf(", ");
                print_ids("noise", sd.noise_read_ids);
                std::printf(", \"haplotype_id\": %u, \"ratio\": %u, \"is_haplotyping_bypassed\": %d}", unsigned(sd.haplotypeId), float_bits(sd.altAlleleHaplotypeCountRatio),
                            sd.isHaplotypingBypassed ? 1 : 0);
            }
            std::printf("]}");
            first = false;
        }
        std::printf("\n]}\n");
    } catch (const std::exception& e) {
        std::fprintf(stderr, "indel_buffer_driver: %s\n", e.what());
        return 1;
    } catch (...) {
        std::fprintf(stderr, "indel_buffer_driver: exception\n");
        return 1;
    }
    return 0;
}
