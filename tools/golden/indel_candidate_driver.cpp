// indel_candidate_driver.cpp -- records what the REFERENCE derives from its IndelBuffer's entries: the two depth buffers per sample, the
// count cache's table, the error model's rate sets, per (key, sample) the four error rates, per key the breakpoint insert size and
// isCandidateIndel: the vectors under tests/golden/indel_candidates/ that anchor tests/indel_candidates_model.py.
//
// TEST INFRASTRUCTURE ONLY; contains no reference code, and is never needed to run the tests: it is built by hand on a machine
// that has the reference tree and the objects oracle/Makefile compiles from it (`make -C oracle ref`):
//
//   L=$REFERENCE/src/c++/lib; O=oracle/_ref
//   g++ -std=c++11 -O2 -w -ffp-contract=off -I$L -Ioracle/ref/gen -Ioracle/boost_shim -I$O/redist/htslib-1.7-6-g6d2bfb7 \
//       -I$O/redist/rapidjson-1.1.0/include -Ioracle/ref tools/golden/indel_candidate_driver.cpp $O/libreftus.a \
//       $O/redist/htslib-1.7-6-g6d2bfb7/libhts.a -lm -lz -lpthread -o $O/bin/indel_candidate_driver
//   python tools/golden/make_indel_candidates_golden.py $O/bin/indel_candidate_driver
//
// The scene goes in as tools/golden/indel_buffer_driver.cpp takes it, and runs the same way: ONE IndelBuffer registered for S samples, the
// reads through addAlignmentIndelsToPosProcessor, then the regions closed in order.  In addition every read's alignment goes into its
// sample's estdepth_buff (iat 0) or estdepth_buff_tier2 (iat 1) through add_alignment_to_depth_buffer, by map level as
// load_read_in_depth_buffer does; the samples are registered with their isCountTowardsDepthFilter; the options below are set.
//
// stdin:   REF, OPT, SAMPLES, BUF, READ, REGION as indel_buffer_driver.cpp
//          MODEL <indel_error_model_name> <isIndelRefErrorFactor> <indelRefErrorFactor> <isHaplotypingEnabled>
//                <is_candidate_indel_signal_test> <min_candidate_indel_open_length>
//          MODELFILE <path>                                        indelErrorModelFilenames: a model file (JSON) instead of the named model; may repeat
//          DEPTHFILTER <maxCandidateDepth>                         IndelBuffer::setMaxCandidateDepth
//          COUNT <sample> <isCountTowardsDepthFilter>
//          WIN <begin> <n_pos>                                     the positions the depth buffers are written out over
//          TIME <repeats>                                          timed: the whole pass, and of it the depth buffers and isCandidateIndel over every key
// stdout:  one JSON document; every double as its bit pattern
#include <limits>
#include <map>
#include <memory>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#define private public // (the count cache's table, the error model's rate sets, the read buffer's range and the indel buffer's map are private members)
#include "starling_common/min_count_binom_gte_cache.hh"
#include "calibration/IndelErrorRateSet.hh"
#include "calibration/IndelErrorModel.hh"
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

void print_rate_set(const char* name, const IndelErrorRateSet& rs)
{
    std::printf("\"%s\": [", name);
    for (size_t i = 0; i < rs._errorRates.size(); ++i) {
        std::printf("%s[", i ? ", " : "");
        for (size_t j = 0; j < rs._errorRates[i].size(); ++j)
            std::printf("%s[%llu, %llu]", j ? ", " : "", double_bits(rs._errorRates[i][j].insertionErrorRate), double_bits(rs._errorRates[i][j].deletionErrorRate));
        std::printf("]");
    }
    std::printf("]");
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
    std::vector<std::string> model_files;
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
        else if (tag == "MODEL") is >> model_name >> is_factor >> factor >> is_haplotyping >> is_signal_test >> min_open_length;
        else if (tag == "DEPTHFILTER") is >> max_candidate_depth;
        else if (tag == "MODELFILE") {
            std::string f;
            is >> f;
            model_files.push_back(f);
        }
        else if (tag == "WIN") is >> win_begin >> win_n;
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
        opt.indelErrorModelFilenames = model_files;
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
        // the whole of a call on a fresh position processor -> the processor, for the map to be read out of
        auto run = [&](double* seconds, double* seconds_candidacy, size_t* n_candidates) {
            RunStatsManager* stats(new RunStatsManager("")); // (kept: the processor refers to it)
            std::unique_ptr<PP> pp(new PP(opt, dopt, ref, streams, n_samples, *stats, count_towards_depth));
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
            const auto t0(std::chrono::steady_clock::now());
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
            const auto t1(std::chrono::steady_clock::now());
            for (size_t i = 0; i < reads.size(); ++i) { // by map level, as load_read_in_depth_buffer does
                const Read& r(reads[i]);
                if (als[i].empty()) continue;
                if (r.iat == INDEL_ALIGN_TYPE::GENOME_TIER1_READ) add_alignment_to_depth_buffer(als[i].pos, als[i].path, pp->depth1(unsigned(r.sample)));
                else if (r.iat == INDEL_ALIGN_TYPE::GENOME_TIER2_READ) add_alignment_to_depth_buffer(als[i].pos, als[i].path, pp->depth2(unsigned(r.sample)));
            }
            size_t n_cand = 0;
            if (seconds) { // (the untimed pass asks below, key by key, while it writes)
                for (const auto& entry : pp->indelBuffer()._indelBuffer) n_cand += pp->indelBuffer().isCandidateIndel(entry.first, entry.second) ? 1 : 0;
            }
            const auto t2(std::chrono::steady_clock::now());
            if (seconds) *seconds += std::chrono::duration<double>(t2 - t0).count();
            if (seconds_candidacy) *seconds_candidacy += std::chrono::duration<double>(t2 - t1).count();
            if (n_candidates) *n_candidates += n_cand;
            return pp;
        };

        if (time_repeats > 0) {
            double seconds = 0, seconds_candidacy = 0;
            size_t sink = 0, n_cand = 0;
            for (int rep = 0; rep < time_repeats; ++rep) sink += run(&seconds, &seconds_candidacy, &n_cand)->indelBuffer()._indelBuffer.size();
            std::printf("{\"time_repeats\": %d, \"reads\": %zu, \"regions\": %zu, \"samples\": %u, \"seconds_per_pass\": %.9f, \"seconds_depth_and_candidacy\": %.9f, "
                        "\"keys\": %zu, \"candidates\": %zu}\n",
                        time_repeats, reads.size(), regions.size(), n_samples, seconds / time_repeats, seconds_candidacy / time_repeats, sink / time_repeats,
                        n_cand / time_repeats);
            return 0;
        }

        std::unique_ptr<PP> pp(run(nullptr, nullptr, nullptr));
        std::printf("{\"papprox\": [");
        for (size_t i = 0; i < dopt.countCache._papprox.size(); ++i) std::printf("%s%llu", i ? ", " : "", double_bits(dopt.countCache._papprox[i]));
        std::printf("], \"log_indel_ref_error_factor\": %llu, \"is_sample_specific\": %d, ", double_bits(dopt.logIndelRefErrorFactor),
                    dopt.getIndelErrorModel()._isUseSampleSpecificErrorRates ? 1 : 0);
        print_rate_set("candidate_rates", dopt.getIndelErrorModel()._candidateErrorRates);
        std::printf(", ");
        std::printf("\"sample_rates\": [");
        for (size_t i = 0; i < dopt.getIndelErrorModel()._sampleErrorRates.size(); ++i) {
            std::printf("%s{", i ? ", " : "");
            print_rate_set("set", dopt.getIndelErrorModel()._sampleErrorRates[i]);
            std::printf("}");
        }
        std::printf("]");
        std::printf(", \"depth\": [");
        for (unsigned s = 0; s < n_samples; ++s) {
            std::printf("%s[", s ? ", " : "");
            for (int which = 0; which < 2; ++which) {
                const depth_buffer& db(which ? pp->depth2(s) : pp->depth1(s));
                std::printf("%s[", which ? ", " : "");
                for (int i = 0; i < win_n; ++i) std::printf("%s%u", i ? ", " : "", db.val(win_begin + i));
                std::printf("]");
            }
            std::printf("]");
        }
        std::printf("], \"keys\": [\n");
        bool first(true);
        for (const auto& entry : pp->indelBuffer()._indelBuffer) { // in the map's order (IndelKey::operator<)
            const IndelKey& key(entry.first);
            const IndelData& data(entry.second);
            std::printf("%s{\"pos\": %d, \"type\": %d, \"del_len\": %u, \"ins\": \"%s\", \"bp_insert_size\": %u, \"is_candidate\": %d, \"rates\": [", first ? "" : ",\n",
                        int(key.pos), int(key.type), unsigned(key.deletionLength), key.insertSequence.c_str(), data.getBreakpointInsertSize(),
                        pp->indelBuffer().isCandidateIndel(key, data) ? 1 : 0);
            for (unsigned s = 0; s < n_samples; ++s) {
                const IndelErrorRates& er(data.getSampleData(s).getErrorRates());
                std::printf("%s[%llu, %llu, %llu, %llu]", s ? ", " : "", double_bits(er.refToIndelErrorProb.getValue()), double_bits(er.indelToRefErrorProb.getValue()),
                            double_bits(er.candidateRefToIndelErrorProb.getValue()), double_bits(er.candidateIndelToRefErrorProb.getValue()));
            }
            std::printf("]}");
            first = false;
        }
        std::printf("\n]}\n");
    } catch (const std::exception& e) {
        std::fprintf(stderr, "indel_candidate_driver: %s\n", e.what());
        return 1;
    } catch (...) {
        std::fprintf(stderr, "indel_candidate_driver: exception\n");
        return 1;
    }
    return 0;
}
