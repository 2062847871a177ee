// active_region_driver.cpp -- records what the REFERENCE's repeat finder and active-region detector compute: the vectors under
// tests/golden/active_region_detect/ that anchor tests/anchor_model.py.
//
// TEST INFRASTRUCTURE ONLY; contains no reference code, and is never needed to run the tests: it is built by hand on a machine
// that has the reference tree and the objects oracle/Makefile compiles from it (`make -C oracle ref`):
//
//   L=$REFERENCE/src/c++/lib; O=oracle/_ref
//   g++ -std=c++11 -O2 -w -ffp-contract=off -I$L -Ioracle/ref/gen -Ioracle/boost_shim -I$O/redist/htslib-1.7-6-g6d2bfb7 \
//       -I$O/redist/rapidjson-1.1.0/include -Ioracle/ref tools/golden/active_region_driver.cpp $O/libreftus.a \
//       $O/redist/htslib-1.7-6-g6d2bfb7/libhts.a -lm -lz -lpthread -o $O/bin/active_region_driver
//   python tools/golden/make_active_region_golden.py $O/bin/active_region_driver   (writes tests/golden/active_region_detect/*.json)
//
// It drives the reference's own ReferenceRepeatFinder (L/starling_common/ReferenceRepeatFinder.hh) the way
// ActiveRegionReadBuffer::setEndPos does (ActiveRegionReadBuffer.cpp:173-189), and its own SampleActiveRegionDetector
// (L/starling_common/ActiveRegionDetector.hh:135-218) with the detector's counters filled through
// ActiveRegionReadBuffer::insertMatch / insertMismatch.
//
// stdin:   REF <offset> <sequence>
//          FINDER <name>                                        a new finder over the current reference
//          REGION <init_pos> <n_head> <n_span> <span pos>...    initRepeatSpan(init_pos), then n_head head positions, on the current finder
//          WALK <name> <win_begin> <n> (<count> <depth>)...     a new detector; updateEndPosition(win_begin + 1 .. win_begin + n)
//          TIME <init_pos> <n_head>                             a fresh finder over n_head head positions, timed on this core
// stdout:  one JSON document
#include <map>
#include <memory>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#define private public // (the finder's ring and the detector's coordinates are private members; first, before any header that includes them)
#include "starling_common/ReferenceRepeatFinder.hh"
#include "starling_common/ActiveRegionReadBuffer.hh"
#include "starling_common/ActiveRegionDetector.hh"
#undef private

#include "options/AlignmentFileOptions.hh"
#include "starling_common/starling_base_shared.hh"

#include <chrono>
#include <cstdio>
#include <iostream>

namespace
{

struct DriverOptions : public starling_base_options
{
    const AlignmentFileOptions& getAlignmentFileOptions() const override
    {
        static AlignmentFileOptions alignFileOpt;
        if (alignFileOpt.alignmentFilenames.empty()) alignFileOpt.alignmentFilenames.push_back("sample.bam");
        return alignFileOpt;
    }
};

const unsigned MaxUnit = ActiveRegionReadBuffer::MaxRepeatUnitLength;
const unsigned BufferSize = ActiveRegionReadBuffer::MaxBufferSize;

void print_row(const std::vector<unsigned>& row)
{
    std::printf("[");
    for (size_t k = 0; k < row.size(); ++k) std::printf("%s%u", k ? "," : "", row[k]);
    std::printf("]");
}

} // namespace

int main()
{
    reference_contig_segment ref;
    std::unique_ptr<ReferenceRepeatFinder> finder;
    bool first_item = true, finder_open = false, first_region = true;
    std::string line;
    std::printf("{\"items\": [\n");
    const auto close_finder = [&]() {
        if (finder_open) std::printf("]}");
        finder_open = false;
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
                close_finder();
                finder.reset();
                ref.seq() = seq;
                ref.set_offset(offset);
            } else if (tag == "FINDER") {
                std::string name;
                is >> name;
                close_finder();
                finder.reset(new ReferenceRepeatFinder(ref, MaxUnit, BufferSize, ActiveRegionReadBuffer::MinRepeatSpan));
                std::printf("%s{\"kind\": \"finder\", \"name\": \"%s\", \"ref_offset\": %d, \"ref\": \"%s\", \"regions\": [\n", first_item ? "" : ",\n", name.c_str(),
                            int(ref.get_offset()), ref.seq().c_str());
                first_item = false;
                finder_open = true;
                first_region = true;
            } else if (tag == "REGION") {
                int init_pos, n_head, n_span;
                is >> init_pos >> n_head >> n_span;
                std::vector<int> span_pos(n_span);
                for (int& p : span_pos) is >> p;
                ReferenceRepeatFinder& f(*finder);
                pos_t m = init_pos - 2 * int(MaxUnit) + 1;
                if (m < ref.get_offset()) m = ref.get_offset();
                const std::vector<unsigned> stale(f._repeatSpan[(m - 1) % f._maxBufferSize]);
                std::map<int, std::vector<unsigned>> rows;
                std::vector<int> anchors;
                f.initRepeatSpan(init_pos);
                // final by now: everything the finder is at least 101 ahead of
                for (pos_t p(m); p <= init_pos - 2; ++p) anchors.push_back(f.isAnchor(p) ? 1 : 0);
                for (const int p : span_pos)
                    if (p >= m && p < init_pos + 2 * int(MaxUnit)) rows[p] = f._repeatSpan[p % f._maxBufferSize];
                for (pos_t pos(init_pos); pos < init_pos + n_head; ++pos) { // setEndPos(pos + 1), then the detector's isAnchor(pos - 1)
                    const pos_t q(pos + 2 * int(MaxUnit));
                    f.updateRepeatSpan(q);
                    for (const int p : span_pos)
                        if (p == q) rows[p] = f._repeatSpan[p % f._maxBufferSize];
                    if (pos - 1 >= m) anchors.push_back(f.isAnchor(pos - 1) ? 1 : 0);
                }
                std::printf("%s{\"init_pos\": %d, \"m\": %d, \"init_span\": ", first_region ? "" : ",\n", init_pos, int(m));
                first_region = false;
                print_row(stale);
                std::printf(", \"anchors\": [");
                for (size_t k = 0; k < anchors.size(); ++k) std::printf("%s%d", k ? "," : "", anchors[k]);
                std::printf("], \"span_pos\": [");
                for (size_t k = 0; k < span_pos.size(); ++k) std::printf("%s%d", k ? "," : "", span_pos[k]);
                std::printf("], \"span_rows\": [");
                for (size_t k = 0; k < span_pos.size(); ++k) {
                    if (k) std::printf(",");
                    print_row(rows.at(span_pos[k]));
                }
                std::printf("]}");
            } else if (tag == "WALK") {
                std::string name;
                int win_begin, n;
                is >> name >> win_begin >> n;
                std::vector<std::pair<unsigned, unsigned>> sites(n);
                for (auto& s : sites) is >> s.first >> s.second;
                close_finder();
                IndelBuffer indels(opt, dopt, ref);
                SampleActiveRegionDetector det(ref, 0.2f, 2, indels);
                ActiveRegionReadBuffer& rb(det._readBuffer);
                std::printf("%s{\"kind\": \"walk\", \"name\": \"%s\", \"ref_offset\": %d, \"ref\": \"%s\", \"win_begin\": %d, \"sites\": [", first_item ? "" : ",\n",
                            name.c_str(), int(ref.get_offset()), ref.seq().c_str(), win_begin);
                first_item = false;
                for (int i = 0; i < n; ++i) std::printf("%s[%u,%u]", i ? "," : "", sites[i].first, sites[i].second);
                std::printf("],\n\"calls\": [");
                for (int i = 0; i < n; ++i) {
                    const pos_t p(win_begin + i);
                    // the ring slot of p, as the intake leaves it before the head reaches p + 1
                    rb._positionToAlignIds[p % BufferSize].clear();
                    rb.resetCounter(p);
                    align_id_t id(0);
                    for (unsigned k = 0; k < sites[i].first; ++k) rb.insertMismatch(id++, p, 'A');
                    for (unsigned k = sites[i].first; k < sites[i].second; ++k) rb.insertMatch(id++, p);
                    const std::unique_ptr<ActiveRegion> r(det.updateEndPosition(p + 1));
                    // [candidate, depth zero, anchor as the call saw them; the six coordinates after the call; the region or -1, -1]
                    std::printf("%s[%d,%d,%d,%d,%d,%d,%d,%d,%u,%d,%d]", i ? "," : "", rb.isCandidateVariant(p) ? 1 : 0, rb.isDepthZero(p) ? 1 : 0, rb.isAnchor(p) ? 1 : 0,
                                det._isBeginning ? 1 : 0, int(det._activeRegionStartPos), int(det._anchorPosFollowingPrevVariant), int(det._prevAnchorPos),
                                int(det._prevVariantPos), det._numVariants, r ? int(r->begin_pos()) : -1, r ? int(r->end_pos()) : -1);
                }
                std::printf("]}");
            } else if (tag == "TIME") {
                int init_pos, n_head;
                is >> init_pos >> n_head;
                close_finder();
                ReferenceRepeatFinder f(ref, MaxUnit, BufferSize, ActiveRegionReadBuffer::MinRepeatSpan);
                const auto t0(std::chrono::steady_clock::now());
                f.initRepeatSpan(init_pos);
                unsigned n_anchor = 0;
                for (pos_t pos(init_pos); pos < init_pos + n_head; ++pos) {
                    f.updateRepeatSpan(pos + 2 * int(MaxUnit));
                    n_anchor += f.isAnchor(pos - 1) ? 1 : 0;
                }
                const double s(std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
                std::printf("%s{\"kind\": \"time\", \"n_head\": %d, \"seconds\": %.6f, \"n_anchor\": %u}", first_item ? "" : ",\n", n_head, s, n_anchor);
                first_item = false;
            }
        }
        close_finder();
        std::printf("\n]}\n");
    } catch (const std::exception& e) {
        std::fprintf(stderr, "active_region_driver: %s\n", e.what());
        return 1;
    } catch (...) {
        std::fprintf(stderr, "active_region_driver: exception\n");
        return 1;
    }
    return 0;
}
