// SlotReader (bonsai_amd/csrc/host/bns_slot_reader.hpp) alone: small files, small pieces, pageable memory (a null context), one
// scenario per run -- tests/test_slot_reader.py.  usage: bns_slot_check <scenario> <scratch directory>; prints key=value lines, exit 0
// when the scenario held.  -DBNS_SLOT_CHECK_STANDALONE: PinnedBuf from malloc, so that the program links against nothing (sanitizer builds).
#include <random>
#include "../../bonsai_amd/csrc/host/bns_slot_reader.hpp"

using namespace bns;

#ifdef BNS_SLOT_CHECK_STANDALONE
char *PinnedBuf::reserve(bns_ctx *, size_t bytes)
{
    if (bytes <= cap) return p;
    release();
    p = static_cast<char *>(std::malloc(bytes)); cap = bytes;
    if (!p) die("out of host memory");
    return p;
}
void PinnedBuf::release() { std::free(p); p = nullptr; cap = 0; }
PinnedBuf::~PinnedBuf() { release(); }
#endif

namespace {
constexpr size_t S = 64u << 10, OVER = 4u << 10, PIECE = 4u << 10;     // slot, overlap, piece
struct Slot { u64 seq = 0; unsigned pieces_left = 0; u64 off[2] = {0, 0}; size_t bytes[2] = {0, 0}; PinnedBuf buf[2]; };
using Reader = SlotReader<Slot>;

struct File {
    std::string data;
    int fd = -1;
    File(const std::string &path, size_t n, unsigned seed)
    {
        std::mt19937 rng(seed);
        data.resize(n);
        for (char &ch : data) ch = (char)rng();
        std::FILE *f = std::fopen(path.c_str(), "wb");
        if (!f || std::fwrite(data.data(), 1, n, f) != n || std::fclose(f) != 0) die("could not write " + path);
        fd = ::open(path.c_str(), O_RDONLY);
        if (fd < 0) die("could not open " + path);
    }
    ~File() { if (fd >= 0) ::close(fd); }
};

// what every scenario shares: the monitor, up to two files, the describe callback (slot seq = S + OVER bytes at seq * S of either file;
// `claim`: the size the reader is told file 0 has)
struct Rig {
    std::mutex mu;
    std::condition_variable cv;
    const File *file[2] = {nullptr, nullptr};
    u64 claim = 0, n_slots = 1;
    unsigned opened = 0;                                       // describe calls (under mu)
    std::function<void(const Slot &)> on_open;                 // (mu held)
    std::unique_ptr<Reader> rd;

    void start(const File *f0, const File *f1, u64 claimed_size)
    {
        file[0] = f0; file[1] = f1; claim = claimed_size;
        n_slots = std::max<u64>(1, (claim + S - 1) / S);
        rd = std::make_unique<Reader>(mu, cv, 4, n_slots, 3, PIECE, "test file", [this](Slot &s, Reader::Plan &p) {
            ++opened;
            for (int i = 0; i < 2; ++i) {
                if (!file[i]) continue;
                const u64 size = i == 0 ? claim : file[i]->data.size();
                s.off[i] = std::min<u64>(s.seq * S, size);
                s.bytes[i] = (size_t)std::min<u64>(size - s.off[i], S + OVER);
                p.span[i] = {file[i]->fd, &s.buf[i], s.off[i], s.bytes[i], S + OVER + 256};
            }
            if (on_open) on_open(s);
        });
    }
    bool same(const Slot &s) const
    {
        for (int i = 0; i < 2; ++i)
            if (file[i] && (s.off[i] + s.bytes[i] > file[i]->data.size() || std::memcmp(s.buf[i].p, file[i]->data.data() + s.off[i], s.bytes[i]) != 0)) return false;
        return true;
    }
    // the consumer: every slot in order, compared with the file(s), given back -> slots that arrived intact (stops at a cancel)
    u64 consume_all()
    {
        u64 good = 0;
        for (u64 seq = 0; seq < n_slots; ++seq) {
            std::unique_ptr<Slot> s;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return rd->cancelled() || rd->loaded(seq); });
                if (rd->cancelled()) break;
                s = rd->take(seq);
            }
            if (s->seq == seq && same(*s)) ++good;
            std::lock_guard<std::mutex> lk(mu);
            rd->give_back(std::move(s));
        }
        return good;
    }
};

int in_order(const std::string &dir)
{
    File f(dir + "/a.bin", 1000003, 1);
    Rig rig;
    rig.start(&f, nullptr, f.data.size());
    const u64 good = rig.consume_all();
    rig.rd->join();                                            // (nobody cancelled: the readers leave by themselves)
    std::printf("slots=%llu good=%llu made=%u cancelled=%d\n", (unsigned long long)rig.n_slots, (unsigned long long)good, rig.rd->slots_made(), (int)rig.rd->cancelled());
    return good == rig.n_slots && rig.rd->slots_made() <= 3 && !rig.rd->cancelled() ? 0 : 1;
}

int two_files(const std::string &dir)
{
    int bad = 0;
    {
        File a(dir + "/a.bin", 300001, 2), b(dir + "/b.bin", 100003, 3);       // (slots 2 .. 4 have no byte of b)
        Rig rig;
        u64 empty_second = 0;
        rig.on_open = [&](const Slot &s) { empty_second += s.bytes[1] == 0; };
        rig.start(&a, &b, a.data.size());
        const u64 good = rig.consume_all();
        rig.rd->join();
        std::printf("slots=%llu good=%llu made=%u empty_second=%llu\n", (unsigned long long)rig.n_slots, (unsigned long long)good, rig.rd->slots_made(), (unsigned long long)empty_second);
        bad += !(good == rig.n_slots && rig.rd->slots_made() <= 3 && empty_second == 3);
    }
    {
        File a(dir + "/a.bin", 0, 4), b(dir + "/b.bin", 0, 5);                 // an empty input: one slot without a piece, loaded as it is
        Rig rig;
        rig.start(&a, &b, 0);
        const u64 good = rig.consume_all();
        rig.rd->join();
        std::printf("empty_slots=%llu empty_good=%llu\n", (unsigned long long)rig.n_slots, (unsigned long long)good);
        bad += !(rig.n_slots == 1 && good == 1);
    }
    return bad;
}

int cancel_blocked(const std::string &dir)
{
    File f(dir + "/a.bin", 1000003, 6);
    Rig rig;
    rig.start(&f, nullptr, f.data.size());
    {
        std::unique_lock<std::mutex> lk(rig.mu);               // nothing is taken: with three slots loaded the readers wait for one to come back
        rig.cv.wait(lk, [&] { return rig.rd->loaded(0) && rig.rd->loaded(1) && rig.rd->loaded(2); });
        rig.rd->cancel();
    }
    rig.rd->join();
    std::printf("joined=1 made=%u opened=%u\n", rig.rd->slots_made(), rig.opened);
    return rig.rd->slots_made() == 3 && rig.opened == 3 ? 0 : 1;
}

int short_read(const std::string &dir)
{
    File f(dir + "/a.bin", 200000, 7);
    Rig rig;
    rig.start(&f, nullptr, f.data.size() + 50000);             // (the file is shorter than the reader is told)
    const u64 good = rig.consume_all();                        // (waits for a slot that never loads: the failure has to wake it)
    rig.rd->join();
    std::lock_guard<std::mutex> lk(rig.mu);
    std::printf("good=%llu cancelled=%d woken=1\nerror=%s\n", (unsigned long long)good, (int)rig.rd->cancelled(), rig.rd->error().c_str());
    return rig.rd->cancelled() && good < rig.n_slots && rig.rd->error() == "short read in test file" ? 0 : 1;
}

int stop_opening(const std::string &dir)
{
    File f(dir + "/a.bin", 1000003, 8);
    Rig rig;
    rig.start(&f, nullptr, f.data.size());
    unsigned opened_at_stop = 0;
    u64 good = 0;
    std::unique_ptr<Slot> kept;
    for (u64 seq = 0; seq < 2; ++seq) {
        std::unique_lock<std::mutex> lk(rig.mu);
        rig.cv.wait(lk, [&] { return rig.rd->loaded(seq); });
        std::unique_ptr<Slot> s = rig.rd->take(seq);
        good += rig.same(*s);
        if (seq == 0) rig.rd->give_back(std::move(s));
        else { kept = std::move(s); rig.rd->stop_opening(); opened_at_stop = rig.opened; }
    }
    rig.rd->join();                                            // (not cancelled: what was loading finishes, then the readers leave)
    std::lock_guard<std::mutex> lk(rig.mu);
    for (u64 seq = 2; seq < rig.opened; ++seq) good += rig.rd->loaded(seq) && rig.same(*rig.rd->peek(seq));
    std::printf("opened_at_stop=%u opened=%u slots=%llu good=%llu cancelled=%d\n", opened_at_stop, rig.opened, (unsigned long long)rig.n_slots, (unsigned long long)good, (int)rig.rd->cancelled());
    return rig.opened == opened_at_stop && rig.opened < rig.n_slots && good == rig.opened && !rig.rd->loaded(rig.opened) && !rig.rd->cancelled() ? 0 : 1;
}
}  // namespace

int main(int argc, char **argv)
{
    alarm(20);                                                 // (a lost wake-up fails the run instead of hanging it)
    if (argc != 3) { std::fprintf(stderr, "usage: %s in_order|two_files|cancel_blocked|short_read|stop_opening <scratch directory>\n", argv[0]); return 2; }
    const std::string what = argv[1], dir = argv[2];
    try {
        if (what == "in_order") return in_order(dir);
        if (what == "two_files") return two_files(dir);
        if (what == "cancel_blocked") return cancel_blocked(dir);
        if (what == "short_read") return short_read(dir);
        if (what == "stop_opening") return stop_opening(dir);
        std::fprintf(stderr, "unknown scenario %s\n", what.c_str());
        return 2;
    } catch (const std::exception &e) { std::fprintf(stderr, "%s\n", e.what()); return 1; }
}
