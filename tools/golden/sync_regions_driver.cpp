// sync_regions_driver.cpp -- records what the REFERENCE's multi-sample ActiveRegionDetector does call by call: the vectors under
// tests/golden/sync_regions/ that anchor tests/sync_model.py.
//
// TEST INFRASTRUCTURE ONLY; contains no reference code, and is never needed to run the tests: it is built by hand on a machine
// that has the reference tree and the objects oracle/Makefile compiles from it (`make -C oracle ref`):
//
//   L=$REFERENCE/src/c++/lib; O=oracle/_ref
//   g++ -std=c++11 -O2 -w -ffp-contract=off -I$L -Ioracle/ref/gen -Ioracle/boost_shim -I$O/redist/htslib-1.7-6-g6d2bfb7 \
//       -I$O/redist/rapidjson-1.1.0/include -Ioracle/ref tools/golden/sync_regions_driver.cpp $O/libreftus.a \
//       $O/redist/htslib-1.7-6-g6d2bfb7/libhts.a -lm -lz -lpthread -o $O/bin/sync_regions_driver
//   python tools/golden/make_sync_regions_golden.py $O/bin/sync_regions_driver   (writes tests/golden/sync_regions/*.json)
//
// It drives the reference's own ActiveRegionDetector (L/starling_common/ActiveRegionDetector.hh:55-130) over S sample read buffers
// whose counters are filled through ActiveRegionReadBuffer::insertMatch / insertMismatch, as active_region_driver.cpp fills one.
// closeActiveRegion runs the reference's processors on those buffers; what they leave in the indel buffer is not recorded.
//
// stdin:   REF <offset> <sequence>
//          BEGIN <name> <n_samples> <default_ploidy>             a new detector over the current reference
//          PLOIDY <sample> <pos> <ploidy>                        updateSamplePloidy
//          STEP <win_begin> <n> (<count> <depth>)...             n pairs per sample, sample by sample; updateEndPosition(win_begin + 1 .. win_begin + n)
//          CLEARBUF <from> <to>                                  ActiveRegionReadBuffer::clearPos(from .. to) on every sample's buffer
//          CLEAR                                                 clear()
// stdout:  one JSON document.  A row, after every call and after clear(), is a string "samples|region|ids": per sample, joined by ';',
//          start, anchor after the last variant, previous anchor, previous variant, number of variants (a leading B: _isBeginning; '=':
//          the coordinates of the row before again; '+': the same with the start and the previous anchor moved along with the call; '^': with
//          the previous anchor alone moved); _synchronizedActiveRegion begin, end, _prevActiveRegionEnd; the id map's runs from,to,id
//          over the 260 positions below _prevActiveRegionEnd where the call moved it (else nothing).  The start and the previous anchor
//          are written as the call's pos minus the coordinate where it is >= 0, -1 otherwise -- at one anchor after the other they stay
//          1 -- the other two as they are.
#include <map>
#include <memory>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#define private public // (the detectors' coordinates and the synchronised region are private members; first, before any header that includes them)
#include "starling_common/ActiveRegionReadBuffer.hh"
#include "starling_common/ActiveRegionDetector.hh"
#undef private

#include "options/AlignmentFileOptions.hh"
#include "starling_common/CandidateSnvBuffer.hh"
#include "starling_common/IndelBuffer.hh"
#include "starling_common/starling_base_shared.hh"

#include <cstdio>
#include <iostream>
#include <stdexcept>

namespace
{

struct DriverOptions : public starling_base_options
{
    const AlignmentFileOptions& getAlignmentFileOptions() const override
    {
        static AlignmentFileOptions alignFileOpt;
        // (one file per sample: the indel error rates are made per file)
        for (int s = int(alignFileOpt.alignmentFilenames.size()); s < 8; ++s) alignFileOpt.alignmentFilenames.push_back("sample" + std::to_string(s) + ".bam");
        return alignFileOpt;
    }
};

const unsigned BufferSize = ActiveRegionReadBuffer::MaxBufferSize;

struct Item
{
    Item(const DriverOptions& opt, const starling_base_deriv_options& dopt, const reference_contig_segment& ref, const unsigned n_samples, const unsigned default_ploidy)
        : depth(n_samples), depth2(n_samples), indels(opt, dopt, ref), snvs(n_samples)
    {
        for (unsigned s = 0; s < n_samples; ++s) indels.registerSample(depth[s], depth2[s], false);
        indels.finalizeSamples();
        det.reset(new ActiveRegionDetector(ref, indels, snvs, opt.maxIndelSize, n_samples, false, default_ploidy));
    }
    std::vector<depth_buffer> depth, depth2;
    IndelBuffer indels;
    CandidateSnvBuffer snvs;
    std::unique_ptr<ActiveRegionDetector> det;
};

int rel(const pos_t at, const pos_t c)
{
    return c < 0 ? -1 : int(at - c);
}

void print_row(ActiveRegionDetector& det, const unsigned n_samples, const pos_t at, const pos_t prev_end_before)
{
    // per sample what the row before said, with the start and the previous anchor as they are and relative to the call: '=' stands for
    // the same coordinates again, '+' for the same with those two moved along with the call, '^' with the previous anchor alone moved
    static std::vector<std::string> last_abs, last_rel, last_mix;
    if (at < 0) {
        last_abs.clear();
        last_rel.clear();
        last_mix.clear();
        return;
    }
    last_abs.resize(n_samples);
    last_rel.resize(n_samples);
    last_mix.resize(n_samples);
    std::printf("\"");
    for (unsigned s = 0; s < n_samples; ++s) {
        const SampleActiveRegionDetector& d(*det._sampleActiveRegionDetector[s]);
        char a[96], r[96], m[96];
        std::snprintf(a, sizeof(a), "%d,%d,%d,%d,%d,%u", d._isBeginning ? 1 : 0, int(d._activeRegionStartPos), int(d._anchorPosFollowingPrevVariant), int(d._prevAnchorPos),
                      int(d._prevVariantPos), d._numVariants);
        std::snprintf(r, sizeof(r), "%s%d,%d,%d,%d,%u", d._isBeginning ? "B" : "", rel(at, d._activeRegionStartPos), int(d._anchorPosFollowingPrevVariant),
                      rel(at, d._prevAnchorPos), int(d._prevVariantPos), d._numVariants);
        std::snprintf(m, sizeof(m), "%d,%d,%d,%d,%d,%u", d._isBeginning ? 1 : 0, int(d._activeRegionStartPos), int(d._anchorPosFollowingPrevVariant), rel(at, d._prevAnchorPos),
                      int(d._prevVariantPos), d._numVariants);
        std::printf("%s%s", s ? ";" : "", last_abs[s] == a ? "=" : last_rel[s] == r ? "+" : last_mix[s] == m ? "^" : r);
        last_mix[s] = m;
        last_abs[s] = a;
        last_rel[s] = r;
    }
    std::printf("|%d,%d,%d|", int(det._synchronizedActiveRegion.begin_pos()), int(det._synchronizedActiveRegion.end_pos()), int(det._prevActiveRegionEnd));
    if (det._prevActiveRegionEnd != prev_end_before) {
        const pos_t hi(det._prevActiveRegionEnd);
        bool first = true;
        pos_t from = 0;
        ActiveRegionId run = -1;
        for (pos_t p(hi - 260); p <= hi; ++p) {
            const ActiveRegionId id(p < hi && p >= 0 ? det.getActiveRegionId(p) : -1);
            if (id == run) continue;
            if (run != -1) {
                std::printf("%s%d,%d,%d", first ? "" : ";", int(from), int(p), int(run));
                first = false;
            }
            run = id;
            from = p;
        }
    }
    std::printf("\"");
}

} // namespace

int main()
{
    reference_contig_segment ref;
    std::unique_ptr<Item> item;
    unsigned n_samples = 0;
    bool first_item = true, first_op = true;
    pos_t last_pos = 0;
    std::string line;
    std::printf("{\"items\": [\n");
    const auto close_item = [&]() {
        if (item) std::printf("]}");
        item.reset();
    };
    try {
        DriverOptions opt;
        opt.isHaplotypingEnabled = true;
        starling_base_deriv_options dopt(opt);
        while (std::getline(std::cin, line)) {
            std::istringstream is(line);
            std::string tag;
            is >> tag;
            if (tag == "REF") {
                int offset;
                std::string seq;
                is >> offset >> seq;
                close_item();
                ref.seq() = seq;
                ref.set_offset(offset);
            } else if (tag == "BEGIN") {
                std::string name;
                unsigned default_ploidy;
                is >> name >> n_samples >> default_ploidy;
                close_item();
                item.reset(new Item(opt, dopt, ref, n_samples, default_ploidy));
                print_row(*item->det, 0, -1, 0); // (a new item: no row before)
                std::printf("%s{\"name\": \"%s\", \"ref_offset\": %d, \"ref\": \"%s\", \"n_samples\": %u, \"default_ploidy\": %u, \"ops\": [\n", first_item ? "" : ",\n",
                            name.c_str(), int(ref.get_offset()), ref.seq().c_str(), n_samples, default_ploidy);
                first_item = false;
                first_op = true;
            } else if (tag == "PLOIDY") {
                unsigned s, ploidy;
                int pos;
                is >> s >> pos >> ploidy;
                item->det->updateSamplePloidy(s, pos, ploidy);
                std::printf("%s{\"op\": \"ploidy\", \"sample\": %u, \"pos\": %d, \"ploidy\": %u}", first_op ? "" : ",\n", s, pos, ploidy);
                first_op = false;
            } else if (tag == "STEP") {
                int win_begin, n;
                is >> win_begin >> n;
                std::vector<std::vector<std::pair<unsigned, unsigned>>> sites(n_samples, std::vector<std::pair<unsigned, unsigned>>(n));
                for (auto& row : sites)
                    for (auto& s : row) is >> s.first >> s.second;
                std::printf("%s{\"op\": \"step\", \"win_begin\": %d,\n\"calls\": [", first_op ? "" : ",\n", win_begin);
                first_op = false;
                // what the calls saw: per sample a digit per position, candidate + 2 * depth zero; the anchors, which must be every sample's
                std::vector<std::string> flags(n_samples);
                std::string anchors;
                for (int i = 0; i < n; ++i) {
                    const pos_t p(win_begin + i);
                    for (unsigned s = 0; s < n_samples; ++s) {
                        // the ring slot of p, as the intake leaves it before the head reaches p + 1
                        ActiveRegionReadBuffer& rb(item->det->getReadBuffer(s));
                        rb._positionToAlignIds[p % BufferSize].clear();
                        rb.resetCounter(p);
                        align_id_t id(0);
                        for (unsigned k = 0; k < sites[s][i].first; ++k) rb.insertMismatch(id++, p, 'A');
                        for (unsigned k = sites[s][i].first; k < sites[s][i].second; ++k) rb.insertMatch(id++, p);
                    }
                    const pos_t before(item->det->_prevActiveRegionEnd);
                    item->det->updateEndPosition(p + 1);
                    last_pos = p + 1;
                    for (unsigned s = 0; s < n_samples; ++s) {
                        const ActiveRegionReadBuffer& rb(item->det->getReadBuffer(s));
                        flags[s] += char('0' + (rb.isCandidateVariant(p) ? 1 : 0) + (rb.isDepthZero(p) ? 2 : 0));
                        if (rb.isAnchor(p) != item->det->getReadBuffer(0).isAnchor(p)) throw std::runtime_error("the samples' finders disagree");
                    }
                    anchors += item->det->getReadBuffer(0).isAnchor(p) ? '1' : '0';
                    std::printf("%s", i ? "," : "");
                    print_row(*item->det, n_samples, last_pos, before);
                }
                std::printf("],\n\"anchors\": \"%s\", \"flags\": [", anchors.c_str());
                for (unsigned s = 0; s < n_samples; ++s) std::printf("%s\"%s\"", s ? "," : "", flags[s].c_str());
                std::printf("]}");
            } else if (tag == "CLEARBUF") {
                int from, to;
                is >> from >> to;
                for (unsigned s = 0; s < n_samples; ++s)
                    for (pos_t p(from); p <= to; ++p) item->det->getReadBuffer(s).clearPos(p);
            } else if (tag == "CLEAR") {
                std::printf("%s{\"op\": \"clear\", \"rel\": %d, \"buf_begin\": [", first_op ? "" : ",\n", int(last_pos));
                first_op = false;
                for (unsigned s = 0; s < n_samples; ++s) std::printf("%s%d", s ? "," : "", int(item->det->getReadBuffer(s).getBeginPos()));
                std::printf("], \"buf_end\": [");
                for (unsigned s = 0; s < n_samples; ++s) std::printf("%s%d", s ? "," : "", int(item->det->getReadBuffer(s).getEndPos()));
                std::printf("], \"after\": ");
                const pos_t before(item->det->_prevActiveRegionEnd);
                item->det->clear();
                print_row(*item->det, n_samples, last_pos, before);
                std::printf("}");
            }
        }
        close_item();
        std::printf("\n]}\n");
    } catch (const std::exception& e) {
        std::fprintf(stderr, "sync_regions_driver: %s\n", e.what());
        return 1;
    } catch (...) {
        std::fprintf(stderr, "sync_regions_driver: exception\n");
        return 1;
    }
    return 0;
}
