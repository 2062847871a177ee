// realign_gate_driver.cpp -- records what the REFERENCE's read realignment asks of a complete IndelBuffer, read by read: get_alignment_zone,
// is_realignable, the return of its own check_for_candidate_indel_overlap, which keys had their candidate status computed by that read's
// gate (the cached status is cleared before every read), which keys hold the read's id in one of their four sets (is_usable_indel's second
// half), and per (key, sample) the bits of the two getLogValue(): the vectors under tests/golden/realign_gate/ that anchor
// tests/realign_gate_model.py.
//
// TEST INFRASTRUCTURE ONLY; contains no reference code, and is never needed to run the tests: it is built by hand on a machine
// that has the reference tree and the objects oracle/Makefile compiles from it (`make -C oracle ref`):
//
//   L=$REFERENCE/src/c++/lib; O=oracle/_ref
//   g++ -std=c++11 -O2 -w -ffp-contract=off -I$L -Ioracle/ref/gen -Ioracle/boost_shim -I$O/redist/htslib-1.7-6-g6d2bfb7 \
//       -I$O/redist/rapidjson-1.1.0/include -Ioracle/ref tools/golden/realign_gate_driver.cpp $O/libreftus.a \
//       $O/redist/htslib-1.7-6-g6d2bfb7/libhts.a -lm -lz -lpthread -o $O/bin/realign_gate_driver
//   python tools/golden/make_realign_gate_golden.py $O/bin/realign_gate_driver
//
// The scene goes in as tools/golden/indel_candidate_driver.cpp takes it and the buffer is made the same way (reads, regions, depth buffers,
// options).  Like oracle/ref/ref_driver_patha.cpp and the reference's own unit test (L/starling_common/test/starling_read_align_test.cpp:22)
// this TU #includes starling_read_align.cpp where it lies to reach its file-static functions.
//
// stdin:   as indel_candidate_driver.cpp (no MODELFILE), and
//          RANGE <sample> <read id> <begin> <end>                  the read's realign_buffer_range (default: [0, 2^30))
//          TIME <repeats>                                          timed: zone, is_realignable, the gate and is_usable_indel over the zone's keys for every read
// stdout:  one JSON document; every double as its bit pattern
#include <limits>
#include <map>
#include <memory>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#define private public // (the read buffer's range and the indel buffer's map are private members)
#include "starling_common/IndelBuffer.hh"
#include "starling_common/ActiveRegionReadBuffer.hh"
#include "starling_common/ActiveRegionProcessor.hh"
#undef private

#include "appstats/RunStatsManager.hh"
#include "blt_util/depth_buffer_util.hh"
#include "options/AlignmentFileOptions.hh"
#include "starling_common/ActiveRegionDetector.hh"
#include "starling_common/CandidateSnvBuffer.hh"
#include "starling_common/starling_base_shared.hh"
#include "starling_common/starling_read_util.hh"
#include "starling_common/starling_streams_base.hh"
#include "starling_common/starling_pos_processor_base.hh"
#include "starling_common/starling_pos_processor_indel_util.hh"

#include "starling_common/starling_read_align.cpp"

#include "htsapi/align_path_bam_util.hh"
#include "starling_common/starling_read.hh"

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
       const unsigned n_samples, RunStatsManager& stats, const std::vector<int>& count_towards_depth)
        : starling_pos_processor_base(opt, dopt, ref, streams, n_samples, stats)
    {
        for (unsigned s = 0; s < n_samples; ++s) {
            sample_info& sif(sample(s));
            getIndelBuffer().registerSample(sif.estdepth_buff, sif.estdepth_buff_tier2, count_towards_depth[s] != 0);
        }
        getIndelBuffer().finalizeSamples();
    }
    void resetRegion(const known_pos_range2& range) { resetRegionBase("chrT", range); }
    IndelBuffer& indelBuffer() { return getIndelBuffer(); }
    CandidateSnvBuffer& candidateSnvBuffer() { return getCandidateSnvBuffer(); }
    depth_buffer& depth1(const unsigned s) { return sample(s).estdepth_buff; }
    depth_buffer& depth2(const unsigned s) { return sample(s).estdepth_buff_tier2; }
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

unsigned long long double_bits(const double x)
{
    unsigned long long u;
    std::memcpy(&u, &x, sizeof(u));
    return u;
}

} // namespace

int main()
{
    std::string ref_seq, model_name("logLinear");
    int ref_offset = 0, time_repeats = 0, win_begin = 0, win_n = 0;
    int is_factor = 0, is_haplotyping = 0, is_signal_test = 1;
    double factor = 1., max_candidate_depth = -1.;
    unsigned max_indel_size = 49, n_samples = 1, min_open_length = 20;
    std::vector<std::pair<int, int>> buf(8, std::make_pair(0, 0));
    std::vector<int> count_towards_depth(8, 1);
    std::vector<Read> reads;
    std::vector<Region> regions;
    std::map<std::pair<int, int>, std::pair<int, int>> ranges;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        std::string tag;
        is >> tag;
        if (tag == "REF") is >> ref_offset >> ref_seq;
        else if (tag == "OPT") is >> max_indel_size;
        else if (tag == "SAMPLES") is >> n_samples;
        else if (tag == "TIME") is >> time_repeats;
        else if (tag == "MODEL") is >> model_name >> is_factor >> factor >> is_haplotyping >> is_signal_test >> min_open_length;
        else if (tag == "DEPTHFILTER") is >> max_candidate_depth;
        else if (tag == "WIN") is >> win_begin >> win_n;
        else if (tag == "RANGE") {
            int s, id, b, e;
            is >> s >> id >> b >> e;
            ranges[std::make_pair(s, id)] = std::make_pair(b, e);
        }
        else if (tag == "COUNT") {
            unsigned s;
            int c;
            is >> s >> c;
            count_towards_depth.at(s) = c;
        } else if (tag == "BUF") {
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
        opt.isHaplotypingEnabled = is_haplotyping != 0;
        opt.maxIndelSize = max_indel_size;
        opt.indel_error_model_name = model_name;
        opt.isIndelRefErrorFactor = is_factor != 0;
        opt.indelRefErrorFactor = factor;
        opt.is_candidate_indel_signal_test = is_signal_test != 0;
        opt.min_candidate_indel_open_length = min_open_length;
        starling_base_deriv_options dopt(opt);
        reference_contig_segment ref;
        ref.seq() = ref_seq;
        ref.set_offset(ref_offset);
        Streams streams(n_samples);
        const std::pair<bool, bool> no_pin(false, false);
        const GlobalAligner<int> aligner(AlignmentScores<int>(ActiveRegionDetector::ScoreMatch, ActiveRegionDetector::ScoreMismatch, ActiveRegionDetector::ScoreOpen,
                                                              ActiveRegionDetector::ScoreExtend, ActiveRegionDetector::ScoreOffEdge, ActiveRegionDetector::ScoreOpen,
                                                              true, true));
        // the buffer, complete: the reads, the regions closed in order, the depth buffers
        std::unique_ptr<PP> pp;
        {
            RunStatsManager* stats(new RunStatsManager("")); // (kept: the processor refers to it)
            pp.reset(new PP(opt, dopt, ref, streams, n_samples, *stats, count_towards_depth));
            pp->resetRegion(known_pos_range2(0, 1000));
            pp->indelBuffer().setMaxCandidateDepth(max_candidate_depth);
            std::vector<bam_record> records(reads.size());
            std::vector<alignment> als(reads.size());
            for (size_t i = 0; i < reads.size(); ++i) {
                const std::vector<uint8_t> qual(reads[i].seq.size(), 30);
                records[i].set_qname("R");
                records[i].set_readqual(reads[i].seq.c_str(), qual.data());
                als[i].pos = reads[i].pos;
                als[i].is_fwd_strand = reads[i].is_fwd != 0;
                for (const auto& s : reads[i].path) als[i].path.push_back(ALIGNPATH::path_segment(static_cast<ALIGNPATH::align_t>(s.first), s.second));
            }
            for (size_t i = 0; i < reads.size(); ++i) {
                const Read& r(reads[i]);
                const bam_seq bseq(records[i].get_bam_read());
                addAlignmentIndelsToPosProcessor(max_indel_size, ref, als[i], bseq, *pp, static_cast<INDEL_ALIGN_TYPE::index_t>(r.iat), static_cast<align_id_t>(r.id),
                                                 unsigned(r.sample), no_pin, r.low_mapq != 0);
            }
            for (unsigned s = 0; s < n_samples; ++s) {
                ActiveRegionReadBuffer& rb(pp->getActiveRegionReadBuffer(s));
                rb._readBufferRange.set_begin_pos(buf[s].first);
                rb._readBufferRange.set_end_pos(buf[s].second);
            }
            for (const Region& g : regions) {
                const known_pos_range2 range(g.begin, g.end);
                for (unsigned s = 0; s < n_samples; ++s) {
                    ActiveRegionReadBuffer& rb(pp->getActiveRegionReadBuffer(s));
                    ActiveRegionProcessor arp(range, g.prev_end, ref, max_indel_size, s, g.ploidy[s], aligner, rb, pp->indelBuffer(), pp->candidateSnvBuffer());
                    arp.processHaplotypes();
                }
            }
            for (size_t i = 0; i < reads.size(); ++i) { // by map level, as load_read_in_depth_buffer does
                const Read& r(reads[i]);
                if (als[i].empty()) continue;
                if (r.iat == INDEL_ALIGN_TYPE::GENOME_TIER1_READ) add_alignment_to_depth_buffer(als[i].pos, als[i].path, pp->depth1(unsigned(r.sample)));
                else if (r.iat == INDEL_ALIGN_TYPE::GENOME_TIER2_READ) add_alignment_to_depth_buffer(als[i].pos, als[i].path, pp->depth2(unsigned(r.sample)));
            }
        }
        const IndelBuffer& ib(pp->indelBuffer());
        for (const auto& entry : ib._indelBuffer) (void)ib.isCandidateIndel(entry.first, entry.second); // (initializeAuxInfo: the rates)
        // the reads as the realignment sees them
        std::vector<std::unique_ptr<starling_read>> sreads;
        for (const Read& r : reads) {
            const std::vector<uint8_t> qual(r.seq.size(), 30);
            bam_record rec;
            rec.set_qname("R");
            rec.set_readqual(r.seq.c_str(), qual.data());
            alignment al;
            al.pos = r.pos;
            al.is_fwd_strand = r.is_fwd != 0;
            for (const auto& s : r.path) al.path.push_back(ALIGNPATH::path_segment(static_cast<ALIGNPATH::align_t>(s.first), s.second));
            bam1_t& br(*(rec.get_data()));
            br.core.pos = al.pos;
            if (!r.is_fwd) br.core.flag |= BAM_FLAG::STRAND;
            edit_bam_cigar(al.path, br);
            const MAPLEVEL::index_t level(r.iat == 0 ? MAPLEVEL::TIER1_MAPPED : (r.iat == 1 ? MAPLEVEL::TIER2_MAPPED : MAPLEVEL::SUB_MAPPED));
            sreads.emplace_back(new starling_read(rec, al, level, static_cast<align_id_t>(r.id)));
        }
        auto range_of = [&](const Read& r) {
            const auto it(ranges.find(std::make_pair(r.sample, r.id)));
            return it == ranges.end() ? known_pos_range(0, 1 << 30) : known_pos_range(it->second.first, it->second.second);
        };
        if (time_repeats > 0) {
            size_t sink = 0;
            const auto t0(std::chrono::steady_clock::now());
            for (int rep = 0; rep < time_repeats; ++rep) {
                for (const auto& entry : ib._indelBuffer) entry.second.status.is_candidate_indel_cached = false;
                for (size_t i = 0; i < reads.size(); ++i) {
                    const read_segment& rseg(sreads[i]->get_full_segment());
                    const known_pos_range zone(getReadAlignmentZone(rseg));
                    if (!rseg.getInputAlignment().is_realignable(opt.maxIndelSize)) continue;
                    sink += check_for_candidate_indel_overlap(range_of(reads[i]), rseg, ib) ? 1 : 0;
                    const auto pair(ib.rangeIterator(zone.begin_pos, zone.end_pos));
                    for (auto it(pair.first); it != pair.second; ++it)
                        sink += is_usable_indel(ib, it->first, getIndelData(it), static_cast<align_id_t>(reads[i].id), unsigned(reads[i].sample)) ? 1 : 0;
                }
            }
            const auto t1(std::chrono::steady_clock::now());
            std::printf("{\"time_repeats\": %d, \"reads\": %zu, \"samples\": %u, \"keys\": %zu, \"seconds_per_pass\": %.9f, \"sink\": %zu}\n", time_repeats, reads.size(), n_samples,
                        ib._indelBuffer.size(), std::chrono::duration<double>(t1 - t0).count() / time_repeats, sink);
            return 0;
        }
        std::printf("{\"keys\": [\n");
        bool first(true);
        for (const auto& entry : ib._indelBuffer) { // in the map's order (IndelKey::operator<)
            const IndelKey& key(entry.first);
            const IndelData& data(entry.second);
            std::printf("%s{\"pos\": %d, \"type\": %d, \"del_len\": %u, \"ins\": \"%s\", \"is_candidate\": %d, \"active_region_id\": %d, \"logs\": [", first ? "" : ",\n", int(key.pos),
                        int(key.type), unsigned(key.deletionLength), key.insertSequence.c_str(), ib.isCandidateIndel(key, data) ? 1 : 0, int(data.activeRegionId));
            for (unsigned s = 0; s < n_samples; ++s) {
                const IndelErrorRates& er(data.getSampleData(s).getErrorRates());
                std::printf("%s[%llu, %llu]", s ? ", " : "", double_bits(er.refToIndelErrorProb.getLogValue()), double_bits(er.indelToRefErrorProb.getLogValue()));
            }
            std::printf("], \"haplotype_id\": [");
            for (unsigned s = 0; s < n_samples; ++s) std::printf("%s%d", s ? ", " : "", int(data.getSampleData(s).haplotypeId));
            std::printf("], \"is_haplotyping_bypassed\": [");
            for (unsigned s = 0; s < n_samples; ++s) std::printf("%s%d", s ? ", " : "", data.getSampleData(s).isHaplotypingBypassed ? 1 : 0);
            std::printf("]}");
            first = false;
        }
        std::printf("\n], \"reads\": [\n");
        for (size_t i = 0; i < reads.size(); ++i) {
            const Read& r(reads[i]);
            const read_segment& rseg(sreads[i]->get_full_segment());
            const known_pos_range zone(getReadAlignmentZone(rseg));
            const known_pos_range range(range_of(r));
            for (const auto& entry : ib._indelBuffer) entry.second.status.is_candidate_indel_cached = false;
            const bool realignable(rseg.getInputAlignment().is_realignable(opt.maxIndelSize));
            const bool gate(realignable && check_for_candidate_indel_overlap(range, rseg, ib));
            std::printf("%s{\"sample\": %d, \"id\": %d, \"zone\": [%d, %d], \"range\": [%d, %d], \"realignable\": %d, \"gate\": %d, \"consulted\": [", i ? ",\n" : "", r.sample, r.id,
                        int(zone.begin_pos), int(zone.end_pos), int(range.begin_pos), int(range.end_pos), realignable ? 1 : 0, gate ? 1 : 0);
            size_t k = 0, n = 0;
            for (const auto& entry : ib._indelBuffer) {
                if (entry.second.status.is_candidate_indel_cached) std::printf("%s%zu", n++ ? ", " : "", k);
                ++k;
            }
            std::printf("], \"member\": [");
            k = n = 0;
            for (const auto& entry : ib._indelBuffer) {
                const IndelSampleData& sd(entry.second.getSampleData(unsigned(r.sample)));
                const align_id_t id(static_cast<align_id_t>(r.id));
                const bool member(sd.tier1_map_read_ids.count(id) > 0 || sd.tier2_map_read_ids.count(id) > 0 || sd.submap_read_ids.count(id) > 0 || sd.noise_read_ids.count(id) > 0);
                const bool usable(is_usable_indel(ib, entry.first, entry.second, id, unsigned(r.sample)));
                if (usable != (member || ib.isCandidateIndel(entry.first, entry.second))) throw std::runtime_error("is_usable_indel is not candidate-or-member");
                if (member) std::printf("%s%zu", n++ ? ", " : "", k);
                ++k;
            }
            std::printf("]}");
        }
        std::printf("\n]}\n");
    } catch (const std::exception& e) {
        std::fprintf(stderr, "realign_gate_driver: %s\n", e.what());
        return 1;
    } catch (...) {
        std::fprintf(stderr, "realign_gate_driver: exception\n");
        return 1;
    }
    return 0;
}
