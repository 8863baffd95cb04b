// bonsai_main.cpp -- `bonsai classify` drop-in (bin/bonsai.cpp:107-163, :521-540) over the MI355X hot path.
#include <dlfcn.h>
#include <getopt.h>
#include <unistd.h>
#include <algorithm>

#include <chrono>
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <thread>
#include <string>
#include <vector>

#include "bns_host.hpp"

namespace {

void usage(const char *exe)
{
    std::fprintf(stderr,
                 "Usage:\n%s classify [flags] <dbpath> <tax_path> <inr1.fq> [<inr2.fq>]\n"
                 "Flags (as bonsai classify):\n"
                 "-o:\tRedirect output to path instead of stdout.\n"
                 "-c:\tSet chunk size in bases per GPU batch. Default: %i\n"
                 "-a:\tEmit all records, not just classified.\n"
                 "-p:\tHost threads for packing reads and formatting output [4, or as many CPUs as there are] (-1: all); the hot path runs on the GPU.\n"
                 "-S:\tper_set (accepted; meaningless without the pthread pool).\n"
                 "-C:\tDo not canonicalize.\n"
                 "-k/-K:\tEmit / do not emit kraken-style output.\n"
                 "-f/-F:\tEmit / do not emit fastq-style output.\n"
                 "Added:\n"
                 "-g:\tGPUs: an index, a range or a list (0, 0-7, 0,2,5, all) [0].  Several GPUs: the db is uploaded once and\n"
                 "\tbroadcast over xGMI (RCCL); every chunk of reads is sharded across them.\n"
                 "-L:\tTable layout in HBM: minbucket (default, minimizer-clustered 128 B buckets), bucket (hashed 64 B buckets)\n"
                 "\tor khash (probe the bns.db arrays as they are).\n"
                 "-P:\tParser threads for one plain (not gzip, not piped) input file [2]: stretches of the file are parsed side by side;\n"
                 "\tn:bytes sets the stretch length.  Output does not depend on it.\n"
                 "-N:\tDo not bind the host threads to the CPUs next to the GPU(s) (the default narrows the affinity mask to them).\n"
                 "-b:\tAlso write every read's (pair's) taxon, in input order, as raw little-endian u32 to this path.\n"
                 "-R:\tAlso write a taxon report to this path after the last read (Kraken 2's standard report layout: percent of all\n"
                 "\treads, clade count, direct count, rank code, taxid, indented name), tallied on the GPU(s).\n"
                 "-n:\tnames.dmp for the report's names (scientific names; without it a taxon is named by its id).\n"
                 "-u:\tWith -R: one more column after the direct count, the number of distinct k-mers of the db that the reads covered in the\n"
                 "\ttaxon's clade (HyperLogLog estimate, 4096 registers: 1.6 %% standard error), by the k-mers' own taxa.\n"
                 "-d:\tWith -R and -u: two more columns after the distinct k-mers, the number of keys the db holds for the taxon's clade (counted on\n"
                 "\tthe GPU from the loaded table) and the coverage, distinct k-mers / db keys.  Not clamped: the numerator is an estimate\n"
                 "\t(1.6 %% standard error) and may exceed 1.\n"
                 "-U:\tTaxa that can have a sketch per GPU context, 4 KiB each [65536]; beyond that a taxon's k-mers are not counted (a warning says so).\n"
                 "-t:\tConfidence threshold in [0, 1] (digits, at most 9 after the point) [0]: a read (pair) is called at the first of its\n"
                 "\ttaxon and the taxon's ancestors whose clade holds at least that fraction of its k-mers, else unclassified.\n"
                 "-M:\tMinimum hit groups, an integer in [0, 64] [0: off]: a read (pair) is called only when at least that many DISTINCT k-mers\n"
                 "\tof it (both mates together) are found in the db; a k-mer found at many positions counts once.  Applied after -t.\n"
                 "-Q:\tMinimum base quality, an integer in [0, 93] [0: off]: a base whose Phred+33 quality is lower counts as N, so no k-mer\n"
                 "\tover it is looked up (FASTQ records; FASTA has no quality).  Not for a read container: mask with `bonsai pack -Q`.\n"
                 "-m:\tMask low-complexity sequence at this level, an integer in [1, 1000] (dustmasker's default: 20) [off]: symmetric DUST,\n"
                 "\twindow 64, over the packed reads on the GPU; a masked base counts as N.  Every input form, a read container included.\n"
                 "\tGive it when the db was built with `bonsai build -m` (a db does not record that).\n"
                 "<inr1.fq> may be a read container written by `bonsai pack` (2-bit reads + names): no parsing, no packing.\n",
                 exe, 1 << 24);
    std::exit(EXIT_FAILURE);
}

// `-t`: a decimal in [0, 1] -- digits, an optional point, at most 9 digits behind it -- parsed exactly into num / 10^d
bool parse_confidence(const char *s, unsigned long long &num, unsigned long long &den)
{
    unsigned long long ip = 0, fp = 0, scale = 1;
    int n_int = 0, n_frac = 0;
    const char *c = s;
    for (; *c >= '0' && *c <= '9'; ++c, ++n_int) { ip = ip * 10 + (unsigned)(*c - '0'); if (ip > 1) return false; }
    if (*c == '.')
        for (++c; *c >= '0' && *c <= '9'; ++c) { if (++n_frac > 9) return false; fp = fp * 10 + (unsigned)(*c - '0'); scale *= 10; }
    if (*c || n_int + n_frac == 0) return false;
    num = ip * scale + fp; den = scale;
    return num <= den;
}

// `-m`: an integer in [1, 1000], digits only
bool parse_dust_level(const char *s, unsigned &level)
{
    unsigned v = 0;
    int n = 0;
    for (; *s >= '0' && *s <= '9'; ++s, ++n) { v = v * 10 + (unsigned)(*s - '0'); if (v > 1000) return false; }
    if (*s || !n || v < 1) return false;
    level = v;
    return true;
}
const char *const DUST_LEVEL_MSG = "[E] -m: the low-complexity level must be an integer in [1, 1000] (dustmasker's default is 20), not '%s'\n";

// `-Q`: an integer in [0, 93], digits only
bool parse_min_quality(const char *s, unsigned &q)
{
    unsigned v = 0;
    int n = 0;
    for (; *s >= '0' && *s <= '9'; ++s, ++n) { v = v * 10 + (unsigned)(*s - '0'); if (v > 93) return false; }
    if (*s || !n) return false;
    q = v;
    return true;
}

// `-M`: an integer in [0, 64], digits only
bool parse_min_hit_groups(const char *s, unsigned &n_min)
{
    unsigned v = 0;
    int n = 0;
    for (; *s >= '0' && *s <= '9'; ++s, ++n) { v = v * 10 + (unsigned)(*s - '0'); if (v > 64) return false; }
    if (*s || !n) return false;
    n_min = v;
    return true;
}

int classify_main(int argc, char *argv[])
{
    int co, num_threads = std::min(4, bns::usable_cpus()), emit_kraken = 1, emit_fastq = 0, emit_all = 0, chunk_size = 1 << 24;
    bool chunk_given = false, bind_cpus = true;
    unsigned parser_threads = 2;
    unsigned long long segment_bytes = 0;
    std::string devices = "0";
    int layout = BNS_LAYOUT_MINBUCKET;
    bool canonicalize = true;
    std::FILE *ofp = stdout, *taxon_fp = nullptr, *report_fp = nullptr;
    const char *names_path = nullptr;
    unsigned long long conf_num = 0, conf_den = 1;
    unsigned min_qual = 0, dust_level = 0, min_hit_groups = 0;
    bool distinct = false, coverage = false;
    long sketch_taxa = 65536;
    if (argc < 4) usage(argv[0]);
    while ((co = getopt(argc, argv, "Cc:p:o:S:afFkKg:L:NP:b:R:n:t:Q:m:M:udU:h?")) >= 0) {
        switch (co) {
            case 'h': case '?': usage(argv[0]); break;
            case 'C': canonicalize = false; break;
            case 'a': emit_all = 1; break;
            case 'c': chunk_size = std::atoi(optarg); chunk_given = true; break;
            case 'F': emit_fastq = 0; break;
            case 'f': emit_fastq = 1; break;
            case 'K': emit_kraken = 0; break;
            case 'k': emit_kraken = 1; break;
            case 'p': num_threads = std::atoi(optarg); if (num_threads < 0) num_threads = bns::usable_cpus(); break;
            case 'o': ofp = std::fopen(optarg, "w"); break;
            case 'b': taxon_fp = std::fopen(optarg, "wb"); if (!taxon_fp) { std::fprintf(stderr, "Could not open taxon file\n"); return EXIT_FAILURE; } break;
            case 'R': report_fp = std::fopen(optarg, "w"); if (!report_fp) { std::fprintf(stderr, "Could not open report file\n"); return EXIT_FAILURE; } break;
            case 'n': names_path = optarg; break;
            case 'u': distinct = true; break;
            case 'd': coverage = true; break;
            case 'U': {
                char *end = nullptr;
                sketch_taxa = std::strtol(optarg, &end, 10);
                if (!*optarg || *end || sketch_taxa < 1 || sketch_taxa > (1L << 20)) {
                    std::fprintf(stderr, "[E] -U: the number of sketched taxa must be an integer in [1, 1048576], not '%s'\n", optarg);
                    return EXIT_FAILURE;
                }
                break;
            }
            case 't':
                if (!parse_confidence(optarg, conf_num, conf_den)) {
                    std::fprintf(stderr, "[E] -t: the confidence threshold must be a decimal in [0, 1] with at most 9 digits after the point, not '%s'\n", optarg);
                    return EXIT_FAILURE;
                }
                break;
            case 'Q':
                if (!parse_min_quality(optarg, min_qual)) {
                    std::fprintf(stderr, "[E] -Q: the minimum base quality must be an integer in [0, 93], not '%s'\n", optarg);
                    return EXIT_FAILURE;
                }
                break;
            case 'm':
                if (!parse_dust_level(optarg, dust_level)) { std::fprintf(stderr, DUST_LEVEL_MSG, optarg); return EXIT_FAILURE; }
                break;
            case 'M':
                if (!parse_min_hit_groups(optarg, min_hit_groups)) {
                    std::fprintf(stderr, "[E] -M: the minimum number of hit groups must be an integer in [0, 64], not '%s'\n", optarg);
                    return EXIT_FAILURE;
                }
                break;
            case 'S': break;
            case 'g': devices = optarg; break;
            case 'N': bind_cpus = false; break;
            case 'P': {
                char *end = nullptr;
                parser_threads = (unsigned)std::max(1L, std::strtol(optarg, &end, 10));
                if (end && *end == ':') segment_bytes = std::strtoull(end + 1, nullptr, 10);
                break;
            }
            case 'L':
                if (std::strcmp(optarg, "khash") == 0) layout = BNS_LAYOUT_KHASH;
                else if (std::strcmp(optarg, "bucket") == 0) layout = BNS_LAYOUT_BUCKET;
                else if (std::strcmp(optarg, "minbucket") == 0) layout = BNS_LAYOUT_MINBUCKET;
                else usage(argv[0]);
                break;
        }
    }
    if (!ofp) { std::fprintf(stderr, "Could not open output file\n"); return EXIT_FAILURE; }
    if (distinct && !report_fp) { std::fprintf(stderr, "[E] -u adds a column to the taxon report: it needs -R <path>\n"); return EXIT_FAILURE; }
    if (coverage && !(distinct && report_fp)) {
        std::fprintf(stderr, "[E] -d adds the db key count and the coverage behind the distinct k-mer column: it needs -R <path> and -u\n");
        usage(argv[0]);
    }
    const int npos = argc - optind;
    if (npos != 3 && npos != 4) usage(argv[0]);
    const auto t_start = std::chrono::steady_clock::now();
    try {
        // (never destroyed, like the classifier below: giving 6.6 GB of arrays back page by page was 0.3 s between the last read and the exit)
        bns::Database &db = *new bns::Database(argv[optind]);
        const auto t_db = std::chrono::steady_clock::now();
        const std::vector<bns::u32> taxmap = bns::build_parent_map(argv[optind + 1]);
        const auto t_tax = std::chrono::steady_clock::now();
        // -g 0-7 / 0,2 / all: one context per GPU, db broadcast over xGMI, whole chunks (2^24 bases unless -c says otherwise) dealt
        // to the devices as they become free
        const std::vector<int> devs = bns::parse_devices(devices.c_str());
        (void)chunk_given;
        if (bind_cpus) {
            const int n = bns::bind_near_devices(devs);
            if (n && std::getenv("BNS_CLI_TIMING")) std::fprintf(stderr, "[timing] threads bound to the %d CPUs next to the GPU(s)\n", n);
        }
        // will the device inflate the input?  (decided here: the waits' mode below must be set before the first context exists)
        bool dev_inflate = false;
        {
            const char *g = std::getenv("BNS_BGZF_GPU");
            unsigned long long bgzf_bytes = 0;
            bool any_bgzf = false;
            for (int a = 2; a < npos; ++a)
                if (bns::is_bgzf_file(argv[optind + a])) {
                    any_bgzf = true;
                    if (std::FILE *f = std::fopen(argv[optind + a], "rb")) { if (std::fseek(f, 0, SEEK_END) == 0) bgzf_bytes += (unsigned long long)std::ftell(f); std::fclose(f); }
                }
            dev_inflate = any_bgzf && (g ? std::atoi(g) != 0 : (bns::usable_cpus() < 12 || bgzf_bytes >= (8ull << 30)));
        }
        // A host thread that waits for the device spins by default (lowest latency) -- one CPU per caller thread for as long as a
        // call lasts, and a call lasts longer when inflate kernels share the device.  When the device inflates the input (below), the
        // waits block instead (the runtime's own switch, set before the first context exists): BGZF +3-6 % on 4-12 CPUs; plain input
        // keeps the spinning waits (blocking: 0 to -7 %).  BNS_BLOCKING_SYNC=0 / 1 by hand.
        {
            const char *e = std::getenv("BNS_BLOCKING_SYNC");
            const bool blocking = e ? std::atoi(e) != 0 : dev_inflate;
            if (blocking) {
                using set_dev_t = int (*)(int);
                using set_flags_t = int (*)(unsigned);
                const auto set_dev = reinterpret_cast<set_dev_t>(::dlsym(RTLD_DEFAULT, "hipSetDevice"));
                const auto set_flags = reinterpret_cast<set_flags_t>(::dlsym(RTLD_DEFAULT, "hipSetDeviceFlags"));
                if (set_dev && set_flags)
                    for (int dv : devs) { (void)set_dev(dv); (void)set_flags(0x4u /* hipDeviceScheduleBlockingSync */); }
            }
        }
        // (never destroyed: the process leaves through _exit when the subcommand returns, and freeing the table, the page-locked
        // buffers and the contexts one by one first was 0.2 s of a 1.5 s run)
        bns::ClassifierGeneric &c = *new bns::ClassifierGeneric(db, taxmap, devs, num_threads, emit_all, emit_fastq, emit_kraken,
                                                                canonicalize, layout);
        c.taxon_out_ = taxon_fp;
        c.report_out_ = report_fp;
        if (conf_num) bns::set_confidence(c, conf_num, conf_den);
        if (min_qual) bns::set_min_base_quality(c, min_qual);
        if (dust_level) bns::set_dust(c, dust_level);
        if (min_hit_groups) bns::set_min_hit_groups(c, min_hit_groups);
        if (report_fp) bns::enable_tally(c);
        if (distinct) bns::enable_sketch(c, (bns::u32)sketch_taxa);
        c.coverage_on_ = coverage;
        if (devs.size() > 1) {                                   // which collective library replicated the db over how many devices
            // (one line per device: a multi-GPU record says what it ran on)
            for (size_t i = 0; i < devs.size(); ++i) {
                char pci[64] = "?";
                (void)bns_device_pci_bus_id(devs[i], pci, (int)sizeof(pci));
                std::string low(pci), numa = "?";
                for (char &ch : low) ch = (char)std::tolower((unsigned char)ch);
                if (std::FILE *nf = std::fopen(("/sys/bus/pci/devices/" + low + "/numa_node").c_str(), "r")) {
                    char nb[32] = {0};
                    if (std::fgets(nb, sizeof(nb), nf)) { numa = nb; while (!numa.empty() && (numa.back() == '\n' || numa.back() == ' ')) numa.pop_back(); }
                    std::fclose(nf);
                }
                std::fprintf(stderr, "context %zu of %zu: device %d (PCI %s, NUMA node %s)\n", i, devs.size(), devs[i], pci, numa.c_str());
            }
            int ver = 0, ranks = 0;
            (void)bns_rccl_info(&ver, &ranks);
            if (ranks) std::fprintf(stderr, "%zu devices: db broadcast by RCCL %d.%d.%d over %d ranks (one upload, xGMI); reads sharded, no collective inside classification\n",
                                    devs.size(), ver / 10000, (ver / 100) % 100, ver % 100, ranks);
            else std::fprintf(stderr, "%zu devices: every device built its table from the host arrays (db too large to replicate array by array, or contexts on one device)\n", devs.size());
        }
        if (std::getenv("BNS_CLI_TIMING"))
            std::fprintf(stderr, "[timing] start-up (db + taxonomy read, context, table load) %.3f s = db file %.3f + nodes.dmp %.3f + contexts, table and taxonomy on the device %.3f\n",
                         std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count(), std::chrono::duration<double>(t_db - t_start).count(),
                         std::chrono::duration<double>(t_tax - t_db).count(), std::chrono::duration<double>(std::chrono::steady_clock::now() - t_tax).count());
        // Blocked-gzip input is inflated on the first device as well (one member per lane; batches taken from the back of the reader's
        // task queue beside the CPU inflaters, or from the front without them) when that pays: on a host short of CPUs (4 CPUs: 3.9 ->
        // 13-22 M reads/s, the device alone; 12: 13 -> 16 M), and on any host when the input is large -- a dozen CPU inflaters are
        // 22 M reads/s, with the device beside them 30-34 M on a 96 M-read file, but its start-up (page-locked staging, the first
        // batches) makes a 32 M-read file a draw (profiles/r04_bgzf_gpu.txt, r04_bgzf_cpus.txt).  BNS_BGZF_GPU=0 / 1 decides it by hand.
        if (dev_inflate && !devs.empty()) bns::set_bgzf_device(devs[0]);
        const auto t_pd = std::chrono::steady_clock::now();
        bns::process_dataset(c, argv[optind + 2], npos == 4 ? argv[optind + 3] : nullptr, ofp, (unsigned)chunk_size, parser_threads, segment_bytes);
        if (std::getenv("BNS_CLI_TIMING"))
            std::fprintf(stderr, "[timing] process_dataset %.3f s\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t_pd).count());
        if (report_fp) {
            const auto t_rep = std::chrono::steady_clock::now();
            bns::write_report(c, taxmap, argv[optind + 1], names_path);
            if (std::getenv("BNS_CLI_TIMING"))
                std::fprintf(stderr, "[timing] report %.3f s\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t_rep).count());
        }
        std::fprintf(stderr, "Classified %llu, unclassified %llu\n", (unsigned long long)c.n_classified(),
                     (unsigned long long)c.n_unclassified());
    } catch (const std::exception &e) {
        std::fprintf(stderr, "[E] %s\n", e.what());
        return EXIT_FAILURE;
    }
    if (ofp != stdout) std::fclose(ofp);
    if (taxon_fp) std::fclose(taxon_fp);
    if (report_fp && std::fclose(report_fp) != 0) { std::fprintf(stderr, "[E] Could not write the report\n"); return EXIT_FAILURE; }
    if (std::getenv("BNS_CLI_TIMING"))
        std::fprintf(stderr, "[timing] since start %.3f s\n",
                     std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count());
    std::fprintf(stderr, "Successfully completed classify!\n");
    return EXIT_SUCCESS;
}

// `bonsai pack`: FASTA / FASTQ (plain or gzip, one file or a pair) -> the pre-packed read container `bonsai classify` takes as it is
// (format: bns_host.hpp).  Host only: no GPU, no db.
int pack_main(int argc, char *argv[])
{
    int co, threads = std::min(8, bns::usable_cpus());
    unsigned parser_threads = 2, chunk = 0;
    bool names = true;
    unsigned min_qual = 0;
    std::string out;
    while ((co = getopt(argc, argv, "o:c:p:P:nQ:h?")) >= 0) {
        switch (co) {
            case 'o': out = optarg; break;
            case 'c': chunk = (unsigned)std::strtoul(optarg, nullptr, 10); break;
            case 'p': threads = std::atoi(optarg); if (threads < 1) threads = bns::usable_cpus(); break;
            case 'P': parser_threads = (unsigned)std::max(1, std::atoi(optarg)); break;
            case 'n': names = false; break;
            case 'Q':
                if (!parse_min_quality(optarg, min_qual)) {
                    std::fprintf(stderr, "[E] -Q: the minimum base quality must be an integer in [0, 93], not '%s'\n", optarg);
                    return EXIT_FAILURE;
                }
                break;
            default:
                std::fprintf(stderr, "Usage: %s pack [-o out.bnsp] [-c bases per chunk (2^27)] [-p pack threads] [-P parser threads] [-n: no read names] "
                                     "[-Q minimum base quality: lower bases packed as N] <in1.fq> [<in2.fq>]\n"
                                     "(no -m: the host packer has no low-complexity mask; `bonsai classify -m` masks a container's reads on the GPU)\n", argv[0]);
                return EXIT_FAILURE;
        }
    }
    const int npos = argc - optind;
    if ((npos != 1 && npos != 2) || out.empty()) {
        std::fprintf(stderr, "Usage: %s pack -o out.bnsp [-c bases per chunk] [-p threads] [-P parser threads] [-n] [-Q min quality] <in1.fq> [<in2.fq>]\n", argv[0]);
        return EXIT_FAILURE;
    }
    try {
        const auto t0 = std::chrono::steady_clock::now();
        const auto r = bns::pack_dataset(argv[optind], npos == 2 ? argv[optind + 1] : nullptr, out.c_str(), chunk, parser_threads, threads, names, min_qual);
        std::fprintf(stderr, "Packed %llu reads, %llu bases in %.2f s\n", (unsigned long long)r.first, (unsigned long long)r.second,
                     std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    } catch (const std::exception &e) {
        std::fprintf(stderr, "[E] %s\n", e.what());
        return EXIT_FAILURE;
    }
    return EXIT_SUCCESS;
}

// `bonsai inspect`: what the db holds per taxon (Kraken 2's kraken2-inspect), counted on the GPU from the table as classify loads it
int inspect_main(int argc, char *argv[])
{
    auto inspect_usage = [&]() {
        std::fprintf(stderr, "Usage: %s inspect [-g device] [-L minbucket|bucket|khash] [-n names.dmp] [-o file] <dbpath> <tax_path>\n"
                             "Prints '# ' lines (k, keys, layout, buckets, window, overflow keys), then the db's keys per taxon in the layout of\n"
                             "classify -R: percent of the db's keys, keys in the clade, keys of the taxon itself, rank code, taxid, name.\n", argv[0]);
        return EXIT_FAILURE;
    };
    int co, device = 0, layout = BNS_LAYOUT_MINBUCKET;
    const char *names_path = nullptr, *out_path = nullptr;
    while ((co = getopt(argc, argv, "g:L:n:o:h?")) >= 0) {
        switch (co) {
            case 'g': device = std::atoi(optarg); break;
            case 'n': names_path = optarg; break;
            case 'o': out_path = optarg; break;
            case 'L':
                if (std::strcmp(optarg, "khash") == 0) layout = BNS_LAYOUT_KHASH;
                else if (std::strcmp(optarg, "bucket") == 0) layout = BNS_LAYOUT_BUCKET;
                else if (std::strcmp(optarg, "minbucket") == 0) layout = BNS_LAYOUT_MINBUCKET;
                else return inspect_usage();
                break;
            default: return inspect_usage();
        }
    }
    if (argc - optind != 2) return inspect_usage();
    std::FILE *ofp = out_path ? std::fopen(out_path, "w") : stdout;
    if (!ofp) { std::fprintf(stderr, "Could not open output file\n"); return EXIT_FAILURE; }
    try {
        bns::Database &db = *new bns::Database(argv[optind]);                // (never destroyed, as in classify)
        const std::vector<bns::u32> taxmap = bns::build_parent_map(argv[optind + 1]);
        bns::ClassifierGeneric &c = *new bns::ClassifierGeneric(db, taxmap, std::vector<int>{device}, 1, 0, 0, 1, true, layout);
        bns::write_inspect(c, db, taxmap, argv[optind + 1], names_path, ofp);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "[E] %s\n", e.what());
        return EXIT_FAILURE;
    }
    if (ofp != stdout && std::fclose(ofp) != 0) { std::fprintf(stderr, "[E] Could not write the inspect report\n"); return EXIT_FAILURE; }
    return EXIT_SUCCESS;
}

// `bonsai distrib`: for every genome, how the db calls each of its windows of read length (what an abundance estimator after Bracken
// needs per db and read length), classified on the GPU with one table lookup per k-mer
int distrib_main(int argc, char *argv[])
{
    auto distrib_usage = [&]() {
        std::fprintf(stderr, "Usage: %s distrib [-l window length: 150] [-t confidence threshold: 0] [-g device] [-L minbucket|bucket|khash]\n"
                             "       [-C: do not canonicalize]\n"
                             "       [-B bases per batch] [-P pairs: slots of the (genome taxid, called taxid) table: 1048576] -M seq2tax [-F paths file]\n"
                             "       [-o file] <dbpath> <tax_path> <genome paths...>\n"
                             "Writes 'mapped_taxid<TAB>genome_taxids:kmers_mapped:total_genome_kmers', then a line per called taxid: the genomes with\n"
                             "windows called there, as <genome taxid>:<windows called here>:<all windows of the genome>.\n"
                             "-t: every window is called as `classify -t` calls it as a read: a decimal in [0, 1] with at most 9 digits after the\n"
                             "    point.  Give the -t (and as -l the read length) of the classify run whose report is to be re-estimated.\n"
                             "(no -m: a window is called as classify calls that substring as a read, and the low-complexity mask of a substring is\n"
                             " not the genome's mask restricted to it)\n", argv[0]);
        return EXIT_FAILURE;
    };
    int co, device = 0, layout = BNS_LAYOUT_MINBUCKET;
    bool canon = true;
    bns::DistribOptions opt;
    std::string seq2taxpath, paths_file;
    const char *out_path = nullptr;
    while ((co = getopt(argc, argv, "l:t:g:L:CB:P:M:F:o:h?")) >= 0) {
        switch (co) {
            case 't': {
                unsigned long long num = 0, den = 1;
                if (!parse_confidence(optarg, num, den)) {
                    std::fprintf(stderr, "[E] -t: the confidence threshold must be a decimal in [0, 1] with at most 9 digits after the point, not '%s'\n", optarg);
                    return distrib_usage();
                }
                opt.conf_num = num; opt.conf_den = den;
                break;
            }
            case 'l': { const long long v = std::atoll(optarg); if (v < 1 || v > 0xFFFFFFFFLL) return distrib_usage(); opt.window_len = (unsigned)v; } break;
            case 'g': device = std::atoi(optarg); break;
            case 'C': canon = false; break;
            case 'B': { const long long v = std::atoll(optarg); if (v < 1) return distrib_usage(); opt.batch_bases = (bns::u64)v; } break;
            case 'P': { const long long v = std::atoll(optarg); if (v < 1 || v > (1LL << 31)) return distrib_usage(); opt.pair_cap = (bns::u32)v; } break;
            case 'M': seq2taxpath = optarg; break;
            case 'F': paths_file = optarg; break;
            case 'o': out_path = optarg; break;
            case 'L':
                if (std::strcmp(optarg, "khash") == 0) layout = BNS_LAYOUT_KHASH;
                else if (std::strcmp(optarg, "bucket") == 0) layout = BNS_LAYOUT_BUCKET;
                else if (std::strcmp(optarg, "minbucket") == 0) layout = BNS_LAYOUT_MINBUCKET;
                else return distrib_usage();
                break;
            default: return distrib_usage();
        }
    }
    if (argc - optind < 2) return distrib_usage();
    std::vector<std::string> inpaths;
    if (!paths_file.empty()) {
        std::FILE *fp = std::fopen(paths_file.c_str(), "r");
        if (!fp) { std::fprintf(stderr, "[E] Could not open %s\n", paths_file.c_str()); return EXIT_FAILURE; }
        char buf[4096];
        while (std::fgets(buf, sizeof(buf), fp)) {
            std::string l(buf);
            while (!l.empty() && (l.back() == '\n' || l.back() == '\r')) l.pop_back();
            if (!l.empty()) inpaths.push_back(l);
        }
        std::fclose(fp);
    } else {
        for (int i = optind + 2; i < argc; ++i) inpaths.emplace_back(argv[i]);
    }
    std::FILE *ofp = nullptr;
    try {
        if (inpaths.empty()) throw bns::Error("Need genome files from command line or file. See usage.");
        if (seq2taxpath.empty()) throw bns::Error("seq2taxpath required: the genomes' taxids come from it. [See -M option.]");
        bns::Database &db = *new bns::Database(argv[optind]);                // (never destroyed, as in classify)
        unsigned comb = db.k_;
        for (bns::u16 g : db.s_) comb += g;
        if (opt.window_len < comb)
            throw bns::Error("-l " + std::to_string(opt.window_len) + ": a window is at least as long as the db's seed (" + std::to_string(comb) + " bases)");
        const std::vector<bns::u32> taxmap = bns::build_parent_map(argv[optind + 1]);
        bns::ClassifierGeneric &c = *new bns::ClassifierGeneric(db, taxmap, std::vector<int>{device}, 1, 0, 0, 1, canon, layout);
        ofp = out_path ? std::fopen(out_path, "w") : stdout;
        if (!ofp) throw bns::Error("Could not open output file");
        bns::write_distrib(c, inpaths, seq2taxpath.c_str(), opt, ofp);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "[E] %s\n", e.what());
        if (ofp && ofp != stdout) { std::fclose(ofp); std::remove(out_path); }
        return EXIT_FAILURE;
    }
    if (ofp != stdout && std::fclose(ofp) != 0) { std::fprintf(stderr, "[E] Could not write the window distribution\n"); return EXIT_FAILURE; }
    return EXIT_SUCCESS;
}

// `bonsai abundance`: a `classify -R` report re-estimated at one level with the `distrib` file of the same db, read length and -t.
// Host code only: no device is opened.
int abundance_main(int argc, char *argv[])
{
    auto abundance_usage = [&]() {
        std::fprintf(stderr, "Usage: bonsai abundance [-l D|K|P|C|O|F|G|S: S] [-T min reads: 10] [-n names.dmp] [-o file] <distrib_file> <report_file> <nodes.dmp>\n"
                             "Re-estimates the reads of a `classify -R` report at one level: a taxon at the level (or below it) keeps its reads, the\n"
                             "reads of a taxon above it go to the level's taxa in proportion to how the db calls their genomes' windows there\n"
                             "(`distrib`, run with the -l read length and the -t of the classify run) times the reads those taxa already have.\n"
                             "-T: a taxon at the level with fewer reads is dropped and its reads are discarded.\n"
                             "Writes name, taxonomy_id, taxonomy_lvl, kraken_assigned_reads, added_reads, new_est_reads, fraction_total_reads;\n"
                             "five totals go to stderr.\n");
        return EXIT_FAILURE;
    };
    int co;
    bns::AbundanceOptions opt;
    const char *names_path = nullptr, *out_path = nullptr;
    while ((co = getopt(argc, argv, "l:T:n:o:h?")) >= 0) {
        switch (co) {
            case 'l': if (std::strlen(optarg) != 1 || !std::strchr("DKPCOFGS", optarg[0])) return abundance_usage(); opt.level = optarg[0]; break;
            case 'T': {
                char *end = nullptr;
                const long long v = std::strtoll(optarg, &end, 10);
                if (!*optarg || *end || v < 0) return abundance_usage();
                opt.min_reads = (bns::u64)v;
                break;
            }
            case 'n': names_path = optarg; break;
            case 'o': out_path = optarg; break;
            default: return abundance_usage();
        }
    }
    if (argc - optind != 3) return abundance_usage();
    std::FILE *ofp = nullptr;
    try {
        double totals[5];
        const std::string text = bns::estimate_abundance_files(argv[optind], argv[optind + 1], argv[optind + 2], names_path, opt, totals);
        ofp = out_path ? std::fopen(out_path, "w") : stdout;
        if (!ofp) throw bns::Error("Could not open output file");
        if (std::fwrite(text.data(), 1, text.size(), ofp) != text.size()) throw bns::Error("Could not write the abundance table");
        std::fprintf(stderr, "reads: %.0f\nunclassified or not in the taxonomy: %.0f\ndiscarded below -T: %.0f\nnot distributed: %.0f\n"
                             "estimated at level %c: %.3f\n", totals[0], totals[1], totals[2], totals[3], opt.level, totals[4]);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "[E] %s\n", e.what());
        if (ofp && ofp != stdout) { std::fclose(ofp); std::remove(out_path); }
        return EXIT_FAILURE;
    }
    if (ofp != stdout && std::fclose(ofp) != 0) { std::fprintf(stderr, "[E] Could not write the abundance table\n"); return EXIT_FAILURE; }
    return EXIT_SUCCESS;
}

// `bonsai build` (bin/bonsai.cpp:169-281, lex / entropy modes): db construction on the GPU.
void build_usage(const char *exe)
{
    std::fprintf(stderr,
                 "Usage: %s build <flags> <out.path> <ignored> <paths>\n"
                 "(positional arguments as bin/bonsai.cpp:214,227 reads them: the db is written to the first, the second is\n"
                 " not used in lex/entropy mode, genome paths start at the third unless -F is given)\nFlags:\n"
                 "-k: Set k. [31]\n-w: Set window size.\n-e: Use entropy maximization (score::Entropy) instead of score::Lex.\n"
                 "-S: Set spacing.\n-T: Set tax_path (nodes.dmp).\n-M: Set seq2taxpath (name<TAB>taxid).\n"
                 "-F: Load genome paths from file.\n-C: Do not canonicalize.\n-z: Write gzip-compressed.\n"
                 "-p: Threads (accepted; the build runs on the GPU).\n-g: GPU index [0].\n"
                 "-B: Bases per batch: the genome files reach the GPU in batches of whole sequences of at most this many bases. [1073741824]\n"
                 "-A: Add to this db (old.bns[.gz]): the new db holds its keys and those of <paths>, as a build over all genomes would.\n"
                 "    k, w and the spacing are taken from the file; a -k, -w or -S that disagrees is an error.  A db records neither -C\n"
                 "    nor -e: repeat them as they were given when the db was built.  <out.path> may be the -A path itself.\n"
                 "-D: Taxonomic-depth minimizers: every window of -w bases keeps the k-mer whose LCA over all genomes lies deepest in\n"
                 "    the taxonomy (then the smaller taxid, then the smaller k-mer).  Reads every genome file twice; excludes -e and -A.\n"
                 "-G: Fewest-genome minimizers: every window of -w bases keeps the k-mer that the fewest genome files hold (then the smaller\n"
                 "    taxid, then the smaller k-mer).  A genome is one input file.  Reads every genome file three times; excludes -e, -D and -A.\n"
                 "-m: Mask low-complexity sequence of the genomes at this level, an integer in [1, 1000] (dustmasker's default: 20) [off]:\n"
                 "    symmetric DUST, window 64, on the GPU; no k-mer over a masked base enters the db.  With -A the added genomes are masked;\n"
                 "    with -D and -G all passes see the same mask.  The db does not record it: classify the reads with the same -m.\n"
                 "-t / -f build the entropy-minimized map the reference builds for them; tax-depth minimisation is -D,\n"
                 "feature-count minimisation is -G.\n", exe);
    std::exit(EXIT_FAILURE);
}

int build_main(int argc, char *argv[])
{
    bns::BuildOptions opt;
    std::string spacing, tax_path, seq2taxpath, paths_file, add_path;
    bool gz = false, k_given = false, w_given = false;
    int c;
    if (argc < 4) build_usage(argv[0]);
    while ((c = getopt(argc, argv, "Cw:M:S:p:k:T:F:g:A:B:m:DGtefzHh?")) >= 0) {
        switch (c) {
            case 'C': opt.canon = false; break;
            case 'D': opt.taxdepth = true; break;
            case 'G': opt.fewest = true; break;
            case 'k': opt.k = (unsigned)std::atoi(optarg); k_given = true; break;
            case 'w': opt.wsz = std::atoi(optarg); w_given = true; break;
            case 'A': add_path = optarg; break;
            case 'B': { const long long v = std::atoll(optarg); if (v < 1) build_usage(argv[0]); opt.batch_bases = (bns::u64)v; } break;
            case 'e': opt.entropy = true; break;
            case 'm':
                if (!parse_dust_level(optarg, opt.dust_level)) { std::fprintf(stderr, DUST_LEVEL_MSG, optarg); return EXIT_FAILURE; }
                break;
            case 'S': spacing = optarg; break;
            case 'T': tax_path = optarg; break;
            case 'M': seq2taxpath = optarg; break;
            case 'F': paths_file = optarg; break;
            case 'z': gz = true; break;
            case 'p': break;
            case 'g': opt.device = std::atoi(optarg); break;
            case 't': case 'f':
                // bin/bonsai.cpp:228 tests `LEX == mode || score_scheme::ENTROPY` -- always true -- and :260-261 then picks
                // lca_map<score::Entropy> for every mode but LEX: -t and -f DO an entropy lca build in the reference.
                opt.entropy = true;
                std::fprintf(stderr, "[W] -%c: the reference's tax-depth / feature-count branch is unreachable (bin/bonsai.cpp:228); "
                                     "building the entropy-minimized lca map it actually builds for this flag\n", c);
                break;
            default: build_usage(argv[0]);
        }
    }
    if (argc - optind < 1) build_usage(argv[0]);
    std::string dbpath = argv[optind];
    const bool has_gz = dbpath.size() > 3 && dbpath.compare(dbpath.size() - 3, 3, ".gz") == 0;
    if (has_gz) gz = true;
    if (gz && !has_gz) { dbpath += ".gz"; std::fprintf(stderr, "Writing gzipped, but without a .gz suffix. Adding it.\n"); }
    std::vector<std::string> inpaths;
    if (!paths_file.empty()) {
        std::FILE *fp = std::fopen(paths_file.c_str(), "r");
        if (!fp) { std::fprintf(stderr, "[E] Could not open %s\n", paths_file.c_str()); return EXIT_FAILURE; }
        char buf[4096];
        while (std::fgets(buf, sizeof(buf), fp)) {
            std::string l(buf);
            while (!l.empty() && (l.back() == '\n' || l.back() == '\r')) l.pop_back();
            if (!l.empty()) inpaths.push_back(l);
        }
        std::fclose(fp);
    } else {
        for (int i = optind + 2; i < argc; ++i) inpaths.emplace_back(argv[i]);
    }
    try {
        if (inpaths.empty()) throw bns::Error("Need input files from command line or file. See usage.");
        if (seq2taxpath.empty()) throw bns::Error("seq2taxpath required for final database generation.");
        if (tax_path.empty()) throw bns::Error("Tax path required. [See -T option.]");
        if (opt.k < 1 || opt.k > 32) throw bns::Error("k must be in [1,32]");
        if (opt.taxdepth && opt.entropy)
            throw bns::Error("-D and -e exclude each other: a window keeps its k-mer by one score, taxonomic depth or entropy");
        if (opt.fewest && opt.entropy)
            throw bns::Error("-G and -e exclude each other: a window keeps its k-mer by one score, the genomes that hold it or entropy");
        if (opt.fewest && opt.taxdepth)
            throw bns::Error("-G and -D exclude each other: a window keeps its k-mer by one score, the genomes that hold it or taxonomic depth");
        if (opt.fewest && !add_path.empty())
            throw bns::Error("-G and -A exclude each other: fewest-genome selection counts every k-mer of every genome, and a db holds neither "
                             "the table of all k-mers it was selected from nor the counts");
        if (opt.taxdepth && !add_path.empty())
            throw bns::Error("-D and -A exclude each other: tax-depth selection scores every k-mer of every genome, and a db does not hold "
                             "the table of all k-mers it was selected from");
        // -A: k, w and the spacing are the file's; what the command line says about them must agree (checked before any device is opened)
        std::unique_ptr<bns::Database> old_db;
        if (!add_path.empty()) {
            old_db.reset(new bns::Database(add_path.c_str()));
            const bns::Database &o = *old_db;
            if (o.k_ < 1 || o.k_ > 32 || o.s_.size() + 1 != o.k_) throw bns::Error("-A " + add_path + ": not a db this build can extend");
            if (k_given && opt.k != o.k_)
                throw bns::Error("-k " + std::to_string(opt.k) + " disagrees with k = " + std::to_string(o.k_) + " of -A " + add_path);
            unsigned comb = o.k_;
            for (bns::u16 g : o.s_) comb += g;
            if (w_given) {
                const unsigned w_eff = (unsigned)std::max<int>((int)comb, std::max<int>(opt.wsz, (int)o.k_));
                if (w_eff != o.w_)
                    throw bns::Error("-w " + std::to_string(opt.wsz) + " (window " + std::to_string(w_eff) + ") disagrees with w = " +
                                     std::to_string(o.w_) + " of -A " + add_path);
            }
            if (!spacing.empty() && bns::parse_spacing(spacing.c_str(), o.k_) != o.s_) {
                std::string have;
                for (size_t i = 0; i < o.s_.size(); ++i) have += (i ? "," : "") + std::to_string(o.s_[i]);
                throw bns::Error("-S " + spacing + " disagrees with the spacing " + have + " of -A " + add_path);
            }
            opt.k = o.k_; opt.wsz = (int)o.w_; opt.spacing = o.s_;
            opt.seed = old_db.get();
        } else {
            opt.spacing = bns::parse_spacing(spacing.c_str(), opt.k);
        }
        const std::vector<bns::u32> taxmap = bns::build_parent_map(tax_path.c_str());
        std::fprintf(stderr, "Final map will be written to %s\n", dbpath.c_str());
        const bns::Database db = bns::lca_map(inpaths, taxmap, seq2taxpath.c_str(), opt);
        // spacing entries as 1 byte each for the plain file (what Database(const char*) reads, database.h:46-48) and
        // 2 bytes each for .gz (what the reference's gz writer emits, database.h:89); this reader takes both
        // (through a temporary file beside it: the db may be the -A file itself, and a failed write leaves no half db under its name)
        const size_t slash = dbpath.rfind('/');
        const std::string tmp = (slash == std::string::npos ? std::string() : dbpath.substr(0, slash + 1)) + ".tmp." +
                                std::to_string((long long)getpid()) + "." + (slash == std::string::npos ? dbpath : dbpath.substr(slash + 1));
        try { db.write(tmp.c_str(), gz ? 2 : 1); } catch (...) { std::remove(tmp.c_str()); throw; }
        if (std::rename(tmp.c_str(), dbpath.c_str()) != 0) { std::remove(tmp.c_str()); throw bns::Error("Could not write " + dbpath); }
        std::fprintf(stderr, "Wrote %llu keys in %llu buckets\n", (unsigned long long)db.db_.size, (unsigned long long)db.db_.n_buckets);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "[E] %s\n", e.what());
        return EXIT_FAILURE;
    }
    return EXIT_SUCCESS;
}

}  // namespace

int main(int argc, char *argv[])
{
    // Everything is written and closed when a subcommand returns; leaving through _exit skips the HIP runtime's exit handlers
    // (0.2-0.3 s of a 1.6 s run on 64 M reads).
    // (BNS_NORMAL_EXIT=1: through exit() -- a profiler that writes its trace from an exit handler needs it)
    auto leave = [](int rc) { std::fflush(stdout); std::fflush(stderr); if (std::getenv("BNS_NORMAL_EXIT")) std::exit(rc); _exit(rc); return rc; };
    // The HIP runtime spreads a process's streams over FOUR hardware queues unless told otherwise, and two streams on one queue take
    // turns: a context has three (kernels, uploads, results), the BGZF path two inflaters more, `-g 0,0` twice that -- an upload
    // stream that shares a queue with the kernels it feeds costs a third of the link rate (bench.py's text leg: 116 -> 171 M reads/s
    // with eight queues).  Before the first HIP call; the caller's own setting wins.
    setenv("GPU_MAX_HW_QUEUES", "8", 0);
    if (argc > 1 && std::strcmp(argv[1], "classify") == 0) return leave(classify_main(argc - 1, argv + 1));
    if (argc > 1 && (std::strcmp(argv[1], "build") == 0 || std::strcmp(argv[1], "phase2") == 0 || std::strcmp(argv[1], "p2") == 0))
        return leave(build_main(argc - 1, argv + 1));                // bin/bonsai.cpp:527-529 aliases
    if (argc > 1 && std::strcmp(argv[1], "pack") == 0) return leave(pack_main(argc - 1, argv + 1));
    if (argc > 1 && std::strcmp(argv[1], "inspect") == 0) return leave(inspect_main(argc - 1, argv + 1));
    if (argc > 1 && std::strcmp(argv[1], "distrib") == 0) return leave(distrib_main(argc - 1, argv + 1));
    if (argc > 1 && std::strcmp(argv[1], "abundance") == 0) return leave(abundance_main(argc - 1, argv + 1));
    std::fprintf(stderr, "Usage: %s <classify|build|pack|inspect|distrib|abundance> ...\n"
                         "  classify <opts> <dbpath> <tax_path> <inr1.fq> [<inr2.fq>]\n"
                         "  build    <opts> <out.path> <ignored> <genome paths>\n"
                         "  pack     -o <out.bnsp> <in1.fq> [<in2.fq>]      (reads -> 2-bit container for classify)\n"
                         "  inspect  <opts> <dbpath> <tax_path>             (the db's keys per taxon, in the layout of classify -R)\n"
                         "  distrib  <opts> <dbpath> <tax_path> <genome paths>  (how the db calls every read-length window of every genome)\n"
                         "  abundance <opts> <distrib_file> <report_file> <nodes.dmp>  (a classify -R report re-estimated at one level)\n"
                         "Other reference subcommands (prebuild, hist, metatree) are out of scope (DESIGN.md).\n", argv[0]);
    return EXIT_FAILURE;
}
