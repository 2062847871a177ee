// The host side of the realignment preamble as a stand-alone program for AddressSanitizer and UndefinedBehaviorSanitizer: sk_debug_realign_preamble_host (the
// core of csrc/preamble_core.h over host arrays), what sk_realign_preamble and sk_realign_preamble_dev refuse before they touch a device, the job's own
// preamble (sk_realign_job_add_read + sk_debug_realign_job_prepared) and sk_realign_job_add_reads_prepared, over the crafted scenes dumped by
// tools/diag/realign_preamble_dump.py.  Every array is a heap block of exactly its size, so a step past an end is seen.  Needs no device.
//
//   python tools/diag/realign_preamble_dump.py /tmp/preamble_scenes.bin
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//       -Iinclude -Istrelka_amd/csrc -x hip strelka_amd/csrc/realign_preamble.hip -x c++ strelka_amd/host/read_realign.cpp tools/diag/realign_preamble_sanitize.cpp \
//       -fsanitize=address,undefined -Lstrelka_amd/lib -lstrelka_amd -Wl,-rpath,$PWD/strelka_amd/lib -o /tmp/preamble_sanitize
//   UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 /tmp/preamble_sanitize /tmp/preamble_scenes.bin
// (the two translation units named on the command line stand before the library's own copies of the same entries)
#include "strelka_amd.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

namespace
{

struct Reader
{
    FILE* f;
    template <typename T> std::unique_ptr<T[]> take(const size_t n)
    {
        std::unique_ptr<T[]> p(new T[n]); // (exactly n: the sanitizer watches both ends)
        if (n && std::fread(p.get(), sizeof(T), n, f) != n) {
            std::fprintf(stderr, "short read\n");
            std::exit(2);
        }
        return p;
    }
    template <typename T> T one() { return take<T>(1)[0]; }
};

struct Sample
{
    int32_t n_reads;
    int64_t path_cap, n_observed, code_cap;
    std::unique_ptr<int32_t[]> pos, n_seg, read_len, realign_begin, realign_end, observed;
    std::unique_ptr<int64_t[]> path_off, observed_off, read_off;
    std::unique_ptr<sk_path_seg[]> path;
    std::unique_ptr<sk_realign_gate_read[]> gate;
    std::unique_ptr<uint8_t[]> code, fwd, status;
};

int fail(const std::string& what)
{
    std::fprintf(stderr, "FAILED: %s\n", what.c_str());
    return 1;
}

} // namespace

int main(int argc, char** argv)
{
    if (argc < 2) return fail("usage: realign_preamble_sanitize SCENES");
    Reader in{ std::fopen(argv[1], "rb") };
    if (!in.f) return fail("cannot open the scenes");
    const int32_t n_scenes = in.one<int32_t>();
    long n_records = 0, n_equal = 0, n_none = 0, n_refused = 0, n_prepared = 0, n_entry_refusals = 0;
    for (int32_t sc = 0; sc < n_scenes; ++sc) {
        const int32_t n_samples = in.one<int32_t>(), max_indel_size = in.one<int32_t>(), ref_offset = in.one<int32_t>(), ref_len = in.one<int32_t>(), hap = in.one<int32_t>();
        const auto ref = in.take<char>(size_t(ref_len));
        const int64_t n_keys = in.one<int64_t>();
        const auto keys = in.take<sk_realign_gate_key>(size_t(n_keys));
        const auto logs = in.take<sk_realign_gate_log_rates>(size_t(n_keys) * size_t(n_samples));
        const int64_t ins_len = in.one<int64_t>();
        const auto ins = in.take<uint8_t>(size_t(ins_len));
        std::vector<Sample> samples(static_cast<size_t>(n_samples));
        std::vector<sk_realign_gate_sample> gs(samples.size());
        std::vector<sk_realign_gate_sample_out> go(samples.size());
        std::vector<sk_realign_preamble_sample> ps(samples.size());
        int64_t n_pass = 0;
        for (size_t s = 0; s < samples.size(); ++s) {
            Sample& m = samples[s];
            m.n_reads = in.one<int32_t>();
            m.path_cap = in.one<int64_t>();
            const size_t n = size_t(m.n_reads);
            m.pos = in.take<int32_t>(n);
            m.path_off = in.take<int64_t>(n);
            m.n_seg = in.take<int32_t>(n);
            m.path = in.take<sk_path_seg>(size_t(m.path_cap));
            m.read_len = in.take<int32_t>(n);
            m.realign_begin = in.take<int32_t>(n);
            m.realign_end = in.take<int32_t>(n);
            m.gate = in.take<sk_realign_gate_read>(n);
            m.observed_off = in.take<int64_t>(n + 1);
            m.n_observed = in.one<int64_t>();
            m.observed = in.take<int32_t>(size_t(m.n_observed));
            m.read_off = in.take<int64_t>(n + 1);
            m.code_cap = in.one<int64_t>();
            m.code = in.take<uint8_t>(size_t(m.code_cap));
            m.fwd = in.take<uint8_t>(n);
            m.status.reset(new uint8_t[n]);
            gs[s] = sk_realign_gate_sample{ m.n_reads, 0, m.pos.get(), m.path_off.get(), m.n_seg.get(), m.path.get(), m.path_cap, m.read_len.get(), nullptr, m.realign_begin.get(),
                                            m.realign_end.get() };
            go[s] = sk_realign_gate_sample_out{ m.gate.get(), m.observed_off.get(), m.observed.get(), m.n_observed };
            ps[s] = sk_realign_preamble_sample{ m.code.get(), m.read_off.get(), m.code_cap, m.fwd.get(), m.status.get() };
            for (size_t r = 0; r < n; ++r) n_pass += m.gate[r].status == SK_RGATE_PASS;
        }
        // the core on the host, into rooms of exactly the passing count
        std::unique_ptr<sk_realign_prepared_read[]> records(new sk_realign_prepared_read[size_t(n_pass)]);
        std::unique_ptr<sk_realign_prepared_source[]> source(new sk_realign_prepared_source[size_t(n_pass)]);
        std::unique_ptr<uint8_t[]> consulted(new uint8_t[size_t(n_keys)]);
        int64_t totals[SK_RPRE_N_TOTALS];
        if (sk_debug_realign_preamble_host(n_samples, gs.data(), go.data(), ps.data(), keys.get(), n_keys, ins.get(), ins_len, ref.get(), ref_offset, ref_len, uint32_t(max_indel_size),
                                           records.get(), source.get(), n_pass, consulted.get(), totals))
            return fail(std::string("sk_debug_realign_preamble_host: ") + sk_last_error());
        n_records += totals[0];
        // what the two entries refuse on the host, before a device is asked for: a record capacity below the passing count, no scratch
        if (n_pass > 0) {
            if (!sk_realign_preamble(n_samples, gs.data(), go.data(), ps.data(), keys.get(), n_keys, ins.get(), ins_len, ref.get(), ref_offset, ref_len, uint32_t(max_indel_size),
                                     records.get(), source.get(), n_pass - 1, consulted.get(), totals))
                return fail("sk_realign_preamble took a record capacity below the passing count");
            ++n_entry_refusals;
        }
        if (!sk_realign_preamble_dev(n_samples, gs.data(), go.data(), ps.data(), keys.get(), totals, n_keys, ins.get(), ins_len, ref.get(), ref_offset, ref_len, uint32_t(max_indel_size),
                                     records.get(), source.get(), n_pass, consulted.get(), totals, nullptr, 0, nullptr))
            return fail("sk_realign_preamble_dev took no scratch");
        ++n_entry_refusals;
        // the job's own preamble, read by read, and the prepared reads
        for (int32_t s = 0; s < n_samples; ++s) {
            const Sample& m = samples[size_t(s)];
            sk_realign_options opt;
            sk_realign_options_default(&opt);
            opt.enumeration = 2;
            opt.sample_count = n_samples;
            opt.max_indel_size = uint32_t(max_indel_size);
            opt.is_haplotyping_enabled = hap;
            sk_realign_job *job = sk_realign_job_create(&opt), *given = sk_realign_job_create(&opt);
            std::vector<sk_indel_info> indels(static_cast<size_t>(n_keys));
            std::vector<std::string> seqs(indels.size());
            for (size_t k = 0; k < indels.size(); ++k) {
                std::memset(&indels[k], 0, sizeof(indels[k]));
                seqs[k].assign(reinterpret_cast<const char*>(ins.get()) + keys[k].ins_off, keys[k].ins_len);
                indels[k].key.pos = keys[k].pos;
                indels[k].key.type = keys[k].type;
                indels[k].key.del_len = keys[k].del_len;
                indels[k].key.ins_len = keys[k].ins_len;
                indels[k].key.ins_seq = seqs[k].c_str();
                indels[k].key.is_candidate = keys[k].is_candidate;
                indels[k].ref_to_indel_log_prob = logs[k * size_t(n_samples) + size_t(s)].ref_to_indel_log_prob;
                indels[k].indel_to_ref_log_prob = logs[k * size_t(n_samples) + size_t(s)].indel_to_ref_log_prob;
                indels[k].active_region_id = keys[k].active_region_id;
                std::memcpy(indels[k].haplotype_id, keys[k].haplotype_id, sizeof(keys[k].haplotype_id));
                std::memcpy(indels[k].is_haplotyping_bypassed, keys[k].is_haplotyping_bypassed, sizeof(keys[k].is_haplotyping_bypassed));
            }
            for (sk_realign_job* j : { job, given })
                if (sk_realign_job_set_reference(j, ref.get(), ref_offset, ref_len) || sk_realign_job_set_indels(j, indels.data(), int32_t(n_keys)))
                    return fail(std::string("job set-up: ") + sk_realign_job_error(j));
            std::vector<sk_read_input> ok_reads;
            std::vector<sk_realign_prepared_read> ok_records;
            std::vector<std::unique_ptr<uint8_t[]>> keep;
            for (int32_t r = 0; r < m.n_reads; ++r) {
                const size_t len = size_t(m.read_len[r]);
                std::unique_ptr<uint8_t[]> code(new uint8_t[len]), qual(new uint8_t[len]);
                for (size_t i = 0; i < len; ++i) {
                    code[i] = int64_t(i) < m.read_off[r + 1] - m.read_off[r] ? m.code[size_t(m.read_off[r]) + i] : uint8_t(SK_BAM_ANY);
                    qual[i] = 30;
                }
                sk_read_input ri;
                std::memset(&ri, 0, sizeof(ri));
                ri.read_code = code.get();
                ri.read_qual = qual.get();
                ri.read_len = m.read_len[r];
                ri.pos = m.pos[r];
                ri.n_seg = m.n_seg[r];
                ri.path = m.path.get() + m.path_off[r];
                ri.is_fwd_strand = m.fwd[r];
                ri.map_level = SK_MAPLEVEL_TIER1;
                ri.sample_index = s;
                ri.realign_begin = m.realign_begin[r];
                ri.realign_end = m.realign_end[r];
                ri.n_observed = int32_t(m.observed_off[r + 1] - m.observed_off[r]);
                ri.observed = m.observed.get() + m.observed_off[r];
                const int at = sk_realign_job_add_read(job, &ri);
                int64_t mine = -1;
                for (int64_t i = 0; i < totals[0] && mine < 0; ++i)
                    if (source[i].sample == s && source[i].read == r) mine = i;
                if (at < 0) {
                    ++n_refused;
                    if (mine >= 0) return fail("a record for a read the job refuses");
                } else {
                    sk_realign_prepared_read theirs;
                    const int rc = sk_debug_realign_job_prepared(job, at, &theirs);
                    if (rc < 0 || (rc == 0) != (mine >= 0)) return fail("scene " + std::to_string(sc) + " read " + std::to_string(r) + ": the job and the core disagree on whether there is a record");
                    if (rc == 0) {
                        if (std::memcmp(&theirs, &records[mine], sizeof(theirs))) return fail("scene " + std::to_string(sc) + " read " + std::to_string(r) + ": the records differ");
                        ++n_equal;
                        ok_reads.push_back(ri);
                        ok_records.push_back(records[mine]);
                    } else {
                        ++n_none;
                    }
                }
                keep.push_back(std::move(code));
                keep.push_back(std::move(qual));
            }
            if (sk_realign_job_add_reads_prepared(given, ok_reads.data(), ok_records.data(), int32_t(ok_reads.size())) != 0)
                return fail(std::string("sk_realign_job_add_reads_prepared: ") + sk_realign_job_error(given));
            n_prepared += long(ok_reads.size());
            if (!ok_records.empty()) { // and what it refuses: a count above the capacity, an index outside the table
                sk_realign_prepared_read bad = ok_records[0];
                bad.n_status = SK_RPRE_K + 1;
                if (sk_realign_job_add_reads_prepared(given, ok_reads.data(), &bad, 1) >= 0) return fail("a status map of 41 entries was taken");
                bad = ok_records[0];
                bad.alignment.lead = int16_t(n_keys);
                if (sk_realign_job_add_reads_prepared(given, ok_reads.data(), &bad, 1) >= 0) return fail("an edge index outside the table was taken");
            }
            sk_realign_job_destroy(job);
            sk_realign_job_destroy(given);
        }
    }
    std::fclose(in.f);
    std::printf("%d scenes: %ld records, %ld equal to the job's byte for byte, %ld reads without a record in both, %ld refused by the job, %ld handed over prepared, "
                "%ld refusals of the entries\n", int(n_scenes), n_records, n_equal, n_none, n_refused, n_prepared, n_entry_refusals);
    return n_records == n_equal ? 0 : fail("records without a counterpart");
}
