// bns_slot_reader.hpp -- the one reader loop under the four device-text pipelines (plain file, pair of plain files, BGZF source, gzip
// source): ranges of one or two files pread into page-locked buffers piece by piece on R threads, a bounded number of buffers ahead of
// whoever takes them, delivered by number and recycled.
#pragma once
#include "bns_host_internal.hpp"

#include <functional>

namespace bns {
constexpr size_t READ_PIECE = 8u << 20;                        // one pread; a slot's pieces are read side by side

// Lives under its OWNER's monitor: the owner's threads wait on conditions that mix the reader's state with their own, so there is one
// mutex and one condition variable, the owner's.  Methods marked (mu held) are called with that mutex locked; every change notifies all.
// Slot: anything with `u64 seq` and `unsigned pieces_left`; the owner's `describe` says what slot `seq` reads and where to.
template <typename Slot>
class SlotReader {
public:
    // up to two spans of a slot (buf == nullptr: none).  `reserve` is apart from `bytes`: a buffer reserved for the largest slot at its
    // first use never grows when it is recycled (PinnedBuf::reserve page-locks what it adds: 0.2-0.45 ms per MiB)
    struct Span { int fd = -1; PinnedBuf *buf = nullptr; u64 off = 0; size_t bytes = 0, reserve = 0; };
    struct Plan { bns_ctx *ctx = nullptr; Span span[2]; };     // ctx: whose device the buffers are page-locked for
    // (mu held) slot.seq is set: fill the plan, reset the slot's own fields
    using Describe = std::function<void(Slot &, Plan &)>;

    double t_read = 0, t_pin = 0;                              // summed over the threads (final after join())

    // n_slots: slots 0 .. n_slots - 1 make up the input; max_slots: slot objects in existence (read ahead + taken + not yet given back)
    SlotReader(std::mutex &mu, std::condition_variable &cv, unsigned n_threads, u64 n_slots, unsigned max_slots, size_t piece, const char *what, Describe describe)
        : mu_(mu), cv_(cv), n_slots_(n_slots), max_slots_(max_slots), piece_(piece), what_(what), describe_(std::move(describe))
    {
        for (unsigned r = 0; r < n_threads; ++r) threads_.emplace_back([this] { loop(); });
    }
    ~SlotReader() { { std::lock_guard<std::mutex> lk(mu_); cancel(); } join(); }
    SlotReader(const SlotReader &) = delete;
    SlotReader &operator=(const SlotReader &) = delete;

    // ---- (mu held)
    bool loaded(u64 seq) const { return loaded_.count(seq) != 0; }
    u64 first_loaded() const { return loaded_.empty() ? ~0ULL : loaded_.begin()->first; }      // (~0: none)
    Slot *peek(u64 seq) const { auto it = loaded_.find(seq); return it == loaded_.end() ? nullptr : it->second.get(); }   // a loaded slot, left where it is
    std::unique_ptr<Slot> take(u64 seq) { auto it = loaded_.find(seq); std::unique_ptr<Slot> s = std::move(it->second); loaded_.erase(it); return s; }   // a LOADED slot, the caller's now
    void give_back(std::unique_ptr<Slot> s) { spare_.push_back(std::move(s)); cv_.notify_all(); }
    void stop_opening() { stopped_ = true; cv_.notify_all(); }   // the slots that are loading finish, no further one is opened
    void cancel() { cancel_ = true; cv_.notify_all(); }
    bool cancelled() const { return cancel_; }
    // the first failure's text is kept; everybody is cancelled and woken (the reader's own threads come here; the owner's may)
    void fail(const std::string &w) { if (error_.empty()) error_ = w; cancel(); }
    const std::string &error() const { return error_; }
    unsigned slots_made() const { return made_; }
    // ---- (mu NOT held) the threads leave when cancelled, or when no slot can be opened any more, none is loading and no piece is queued
    void join() { for (auto &t : threads_) if (t.joinable()) t.join(); }

private:
    struct Piece { Slot *slot; int fd; char *dst; size_t len; u64 at; };

    // (mu held on entry and exit, dropped around the page-locking) the next slot: from the spare ones or a new one, described, reserved, cut into pieces
    void open(std::unique_lock<std::mutex> &lk)
    {
        std::unique_ptr<Slot> owned;
        if (!spare_.empty()) { owned = std::move(spare_.back()); spare_.pop_back(); }
        else { owned = std::make_unique<Slot>(); ++made_; }
        Slot *s = owned.get();
        const u64 seq = s->seq = next_++;
        Plan plan;
        describe_(*s, plan);
        loading_[seq] = std::move(owned);
        lk.unlock();
        const double t0 = tnow();
        for (const Span &sp : plan.span) if (sp.buf) sp.buf->reserve(plan.ctx, sp.reserve);
        const double t1 = tnow();
        lk.lock();
        t_pin += t1 - t0;
        unsigned np = 0;
        for (const Span &sp : plan.span)
            for (size_t o = 0; sp.buf && o < sp.bytes; o += piece_) { pieces_.push_back(Piece{s, sp.fd, sp.buf->p + o, std::min(piece_, sp.bytes - o), sp.off + o}); ++np; }
        s->pieces_left = np;
        if (!np) deliver(seq);                                  // (an empty input: its one slot is loaded as it is)
        cv_.notify_all();
    }
    void deliver(u64 seq) { auto it = loading_.find(seq); loaded_[seq] = std::move(it->second); loading_.erase(it); }

    void loop()
    {
        try {
            for (;;) {
                Piece pc{};
                {
                    std::unique_lock<std::mutex> lk(mu_);
                    for (;;) {
                        if (cancel_) return;
                        if (!pieces_.empty()) { pc = pieces_.front(); pieces_.pop_front(); break; }
                        const bool more = !stopped_ && next_ < n_slots_;
                        if (more && (!spare_.empty() || made_ < max_slots_)) { open(lk); continue; }
                        if (!more && loading_.empty()) return;
                        cv_.wait(lk);
                    }
                }
                const double t0 = tnow();
                pread_all(pc.fd, pc.dst, pc.len, pc.at, what_);
                const double t1 = tnow();
                std::lock_guard<std::mutex> lk(mu_);
                t_read += t1 - t0;
                if (--pc.slot->pieces_left == 0) deliver(pc.slot->seq);
                cv_.notify_all();
            }
        } catch (const std::exception &e) { std::lock_guard<std::mutex> lk(mu_); fail(e.what()); }
    }

    std::mutex &mu_;
    std::condition_variable &cv_;
    const u64 n_slots_;
    const unsigned max_slots_;
    const size_t piece_;
    const char *what_;                                         // pread_all's "short read in <what>"
    Describe describe_;
    std::vector<std::unique_ptr<Slot>> spare_;
    unsigned made_ = 0;
    std::deque<Piece> pieces_;                                 // reads to do
    std::map<u64, std::unique_ptr<Slot>> loading_, loaded_;
    u64 next_ = 0;
    bool cancel_ = false, stopped_ = false;
    std::string error_;
    std::vector<std::thread> threads_;
};
}  // namespace bns
