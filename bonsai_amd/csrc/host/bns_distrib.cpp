// bns_distrib.cpp -- `bonsai distrib`: every window of read length of every genome, called by the loaded db on the device (the window
// session of the device library, bns_windows_begin_conf ..: `-t` is the session's threshold), and the per-genome distribution of those calls as a text file.
#include "bns_host_internal.hpp"

namespace bns {

std::string format_distrib(const u32 *seq_taxid, const u32 *called, const u64 *count, u64 n_pairs)
{
    std::map<u32, u64> total;                                   // all windows of a genome taxid
    std::map<u32, std::map<u32, u64>> lines;                    // called taxid -> genome taxid -> windows
    for (u64 i = 0; i < n_pairs; ++i) {
        total[seq_taxid[i]] += count[i];
        if (called[i]) lines[called[i]][seq_taxid[i]] += count[i];
    }
    std::string s = "mapped_taxid\tgenome_taxids:kmers_mapped:total_genome_kmers\n";
    for (const auto &line : lines) {
        s += std::to_string(line.first);
        char sep = '\t';
        for (const auto &e : line.second) {
            s += sep; sep = ' ';
            s += std::to_string(e.first); s += ':'; s += std::to_string(e.second); s += ':'; s += std::to_string(total[e.first]);
        }
        s += '\n';
    }
    return s;
}

void write_distrib(ClassifierGeneric &c, const std::vector<std::string> &paths, const char *seq2tax_path, const DistribOptions &opt, std::FILE *out)
{
    const auto names = build_name_hash(seq2tax_path);
    bns_ctx *ctx = c.ctx_;
    chk(ctx, bns_windows_begin_conf(ctx, opt.window_len, opt.pair_cap, opt.conf_num, opt.conf_den), "bns_windows_begin_conf");
    struct End { bns_ctx *c; ~End() { bns_windows_end(c); } } end{ctx};

    BatchQueue q;
    std::thread reader([&] { read_build_batches(paths, names, opt.batch_bases ? opt.batch_bases : 1, q); });
    struct Join { BatchQueue &q; std::thread &t; ~Join() { q.abandon(); if (t.joinable()) t.join(); } } join{q, reader};

    GrowMem d_bases(ctx), d_off(ctx), d_tx(ctx);
    BuildBatch b;
    u64 n_windows = 0;
    double t_wait = 0, t_upload = 0, t_add = 0;                  // seconds of this thread (BNS_CLI_TIMING)
    for (;;) {
        const double tw0 = tnow();
        const bool more = q.pop(b);                              // (the reader is already at the batch after this one)
        t_wait += tnow() - tw0;
        if (!more) break;
        const u64 total = b.offsets.back();
        for (size_t i = 0; i + 1 < b.offsets.size(); ++i) {
            const u64 n = b.offsets[i + 1] - b.offsets[i];
            if (n >= opt.window_len) n_windows += n - opt.window_len + 1;
        }
        b.bases.resize(b.bases.size() + 8, 'N');                 // readable tail
        const double tu0 = tnow();
        d_bases.ensure(b.bases.size()); d_off.ensure(b.offsets.size() * 8); d_tx.ensure(b.taxids.size() * 4);
        chk(ctx, bns_dev_upload(ctx, d_bases.p, b.bases.data(), b.bases.size()), "upload");
        chk(ctx, bns_dev_upload(ctx, d_off.p, b.offsets.data(), b.offsets.size() * 8), "upload");
        chk(ctx, bns_dev_upload(ctx, d_tx.p, b.taxids.data(), b.taxids.size() * 4), "upload");
        std::string().swap(b.bases);
        t_upload += tnow() - tu0;
        const double ta0 = tnow();
        chk(ctx, bns_windows_add(ctx, (const char *)d_bases.p, (const u64 *)d_off.p, b.taxids.size(), total, (const u32 *)d_tx.p, nullptr, nullptr),
            "bns_windows_add");
        chk(ctx, bns_dev_sync(ctx), "bns_dev_sync");             // the batch's buffers are written again by the next upload
        t_add += tnow() - ta0;
    }
    q.rethrow();

    u64 n_pairs = 0, n_dropped = 0;
    int rc = bns_windows_read(ctx, nullptr, nullptr, nullptr, 0, &n_pairs, &n_dropped, 0);
    chk(ctx, rc, "bns_windows_read");
    if (n_dropped)
        die(std::to_string(n_dropped) + " of " + std::to_string(n_windows) + " windows found no slot in the pair table of " +
            std::to_string(opt.pair_cap) + " slots: give it more with -P pairs");
    std::vector<u32> seq(n_pairs), called(n_pairs);
    std::vector<u64> count(n_pairs);
    chk(ctx, bns_windows_read(ctx, seq.data(), called.data(), count.data(), n_pairs, &n_pairs, &n_dropped, 0), "bns_windows_read");
    const std::string text = format_distrib(seq.data(), called.data(), count.data(), n_pairs);
    if (std::fwrite(text.data(), 1, text.size(), out) != text.size()) die("Could not write the window distribution");
    if (std::getenv("BNS_CLI_TIMING"))
        std::fprintf(stderr, "[timing] distrib: %llu windows, waiting for the reader %.3f s, upload %.3f s, window session %.3f s\n",
                     (unsigned long long)n_windows, t_wait, t_upload, t_add);
}

}  // namespace bns
