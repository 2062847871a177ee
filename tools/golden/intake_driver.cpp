// intake_driver.cpp -- records what the REFERENCE's read intake derives from a set of reads: the vectors under
// tests/golden/read_intake/ that anchor tests/intake_model.py.
//
// TEST INFRASTRUCTURE ONLY; contains no reference code, and is never needed to run the tests: it is built by hand on a machine
// that has the reference tree and the objects oracle/Makefile compiles from it (`make -C oracle ref`):
//
//   L=$REFERENCE/src/c++/lib; O=oracle/_ref
//   g++ -std=c++11 -O2 -w -ffp-contract=off -I$L -Ioracle/ref/gen -Ioracle/boost_shim -I$O/redist/htslib-1.7-6-g6d2bfb7 \
//       -I$O/redist/rapidjson-1.1.0/include -Ioracle/ref tools/golden/intake_driver.cpp $O/libreftus.a \
//       $O/redist/htslib-1.7-6-g6d2bfb7/libhts.a -lm -lz -lpthread -o $O/bin/intake_driver
//   python tools/golden/make_intake_golden.py $O/bin/intake_driver        (writes tests/golden/read_intake/intake_golden.json.gz)
//
// A minimal subclass of starling_pos_processor_base (L/starling_common/starling_pos_processor_base.hh:86) with haplotyping on, so
// that addAlignmentIndelsToPosProcessor (L/starling_common/starling_pos_processor_indel_util.cpp:300-491) feeds the active-region
// detector's read buffer.  The function is called directly, read by read; the head position is never advanced, so no stage runs and
// nothing clears the detector's ring of 1 000 positions (the caller keeps every position inside [0, 1000)).
//   * per read, in a processor reset for that read alone: the valid range (get_valid_alignment_range called as the function calls
//     it), the returned span, and the IndelBuffer walked for the read's observations;
//   * after all reads in one processor: _variantCounter, _depth and isCandidateVariant of every position.
//
// stdin:   REF <offset> <sequence>
//          OPT <max_indel_size>
//          READ <pos> <is_low_mapq> <sequence> <n_seg> (<type> <length>)...      type = ALIGNPATH::align_t
//          SITES <begin> <end>
// stdout:  one JSON document
#include <map>
#include <memory>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#define private public // (the detector's counters are private members; first, before any header that includes this one)
#include "starling_common/ActiveRegionReadBuffer.hh"
#undef private

#include "appstats/RunStatsManager.hh"
#include "options/AlignmentFileOptions.hh"
#include "starling_common/starling_base_shared.hh"
#include "starling_common/starling_read_util.hh"
#include "starling_common/starling_streams_base.hh"
#include "starling_common/starling_pos_processor_base.hh"
#include "starling_common/starling_pos_processor_indel_util.hh"

#include <cstdio>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

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
    int pos, low_mapq;
    std::string seq;
    std::vector<std::pair<int, unsigned>> path;
};

void fill(const Read& r, bam_record& br, alignment& al)
{
    const std::vector<uint8_t> qual(r.seq.size(), 30);
    br.set_qname("R");
    br.set_readqual(r.seq.c_str(), qual.data());
    al.pos = r.pos;
    al.is_fwd_strand = true;
    for (const auto& s : r.path) al.path.push_back(ALIGNPATH::path_segment(static_cast<ALIGNPATH::align_t>(s.first), s.second));
}

} // namespace

int main()
{
    std::string ref_seq;
    int ref_offset = 0, site_begin = 0, site_end = 0;
    unsigned max_indel_size = 49;
    std::vector<Read> reads;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        std::string tag;
        is >> tag;
        if (tag == "REF") is >> ref_offset >> ref_seq;
        else if (tag == "OPT") is >> max_indel_size;
        else if (tag == "SITES") is >> site_begin >> site_end;
        else if (tag == "READ") {
            Read r;
            int n_seg = 0;
            is >> r.pos >> r.low_mapq >> r.seq >> n_seg;
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
        const known_pos_range2 region(site_begin, site_end);
        const std::pair<bool, bool> no_pin(false, false);

        std::printf("{\"ref_offset\": %d, \"ref\": \"%s\", \"max_indel_size\": %u, \"reads\": [\n", ref_offset, ref_seq.c_str(), max_indel_size);
        for (size_t i = 0; i < reads.size(); ++i) {
            const Read& r(reads[i]);
            pp.resetRegion(region);
            bam_record br;
            alignment al;
            fill(r, br, al);
            const bam_seq bseq(br.get_bam_read());
            pos_range valid;
            {
                const rc_segment_bam_seq ref_bseq(ref);
                get_valid_alignment_range(al, ref_bseq, bseq, valid);
            }
            const align_id_t id(static_cast<align_id_t>(i));
            const unsigned span = addAlignmentIndelsToPosProcessor(max_indel_size, ref, al, bseq, pp, INDEL_ALIGN_TYPE::GENOME_TIER1_READ, id, 0, no_pin,
                                                                   r.low_mapq != 0);
            std::printf("{\"pos\": %d, \"low_mapq\": %d, \"seq\": \"%s\", \"path\": [", r.pos, r.low_mapq, r.seq.c_str());
            for (size_t k = 0; k < r.path.size(); ++k) std::printf("%s[%d, %u]", k ? ", " : "", r.path[k].first, r.path[k].second);
            std::printf("], \"valid\": [%d, %d], \"span\": %u, \"obs\": [", valid.begin_pos, valid.end_pos, span);
            bool first = true;
            const auto range(pp.indels().rangeIterator(-100000, 100000));
            for (auto it(range.first); it != range.second; ++it) {
                const IndelKey& k(it->first);
                const IndelData& d(it->second);
                const IndelSampleData& sd(d.getSampleData(0));
                const bool in_noise(sd.noise_read_ids.count(id) != 0), in_tier1(sd.tier1_map_read_ids.count(id) != 0);
                if (!in_noise && !in_tier1) continue;
                std::printf("%s{\"pos\": %d, \"type\": %d, \"deletion_length\": %u, \"ins\": \"%s\", \"bp\": \"%s\", \"is_noise\": %d}", first ? "" : ", ",
                            k.pos, int(k.type), k.deletionLength, k.insertSequence.c_str(),
                            k.is_breakpoint() ? d.getBreakpointInsertSeq().c_str() : "", in_noise ? 1 : 0);
                first = false;
            }
            std::printf("]}%s\n", i + 1 < reads.size() ? "," : "");
        }
        // all the reads into one detector
        pp.resetRegion(region);
        for (size_t i = 0; i < reads.size(); ++i) {
            bam_record br;
            alignment al;
            fill(reads[i], br, al);
            const bam_seq bseq(br.get_bam_read());
            addAlignmentIndelsToPosProcessor(max_indel_size, ref, al, bseq, pp, INDEL_ALIGN_TYPE::GENOME_TIER1_READ, static_cast<align_id_t>(i), 0, no_pin,
                                             reads[i].low_mapq != 0);
        }
        const ActiveRegionReadBuffer& rb(pp.getActiveRegionReadBuffer(0));
        std::printf("], \"site_begin\": %d, \"sites\": [\n", site_begin);
        for (int p = site_begin; p < site_end; ++p)
            std::printf("[%u, %u, %d]%s", rb._variantCounter[p % ActiveRegionReadBuffer::MaxBufferSize], rb._depth[p % ActiveRegionReadBuffer::MaxBufferSize],
                        rb.isCandidateVariant(p) ? 1 : 0, p + 1 < site_end ? ", " : "");
        std::printf("]}\n");
    } catch (const std::exception& e) {
        std::fprintf(stderr, "intake_driver: %s\n", e.what());
        return 1;
    } catch (...) {
        std::fprintf(stderr, "intake_driver: exception\n");
        return 1;
    }
    return 0;
}
