// operators.cpp -- the hot-path operators as host-side state machines (same names, call protocol and error behaviour as
// the reference's Java operators; the work inside addInput / getOutput runs in the gfx950 kernels).
#include "operators.h"

#include <algorithm>
#include <array>
#include <deque>
#include <map>
#include <set>

#include "kernels.h"

#include <cstdlib>
#include <cstring>

namespace tgpu {

// May an operator keep `in` by reference after add_input returned and launch its kernels in a LATER call?  Library-owned pages (another
// operator's output handed over as such, an ingested host page) hold their buffers.  A page that came in as TGPU_DEVICE blocks (`blocks`)
// is the caller's to judge: only its promise (tgpu_context_set_device_input_stable) defers the launches -- also when ingest found the
// owners of its blocks (Context::owner_of): shared owners replace COPIES (the hash builder, the pass-through operators), they do not
// change in which call an operator reads the caller's blocks.
static bool page_is_retained(Context *ctx, const DevicePage &in, const tgpu_page *blocks)
{
    if (ctx->device_input_stable()) return true;
    if (blocks)
        for (int32_t ch = 0; ch < blocks->channel_count; ch++)
            if (blocks->blocks[ch].encoding == TGPU_FLAT && blocks->blocks[ch].memory == TGPU_DEVICE) return false;
    for (const DeviceColumn &c : in.cols) {
        if (c.n > 0 && !c.values_buf) return false;
        if (c.nulls && !c.nulls_buf) return false;
        if (c.offsets && !c.offsets_buf) return false;
    }
    return true;
}

// ---- what the operators below share ---------------------------------------------------------------------------------------------------
namespace {
std::vector<int32_t> types_of_channels(const std::vector<int32_t> &types, const std::vector<int32_t> &channels)
{
    std::vector<int32_t> out;
    for (int32_t ch : channels) out.push_back(types[(size_t)ch]);
    return out;
}

void check_page_types(const DevicePage &in, const std::vector<int32_t> &types)
{
    TG_CHECK_ARG(in.cols.size() == types.size(), "page channel count does not match the operator's types");
    for (size_t i = 0; i < types.size(); i++) TG_CHECK_ARG(in.cols[i].type == types[i], "page channel type does not match the operator's types");
}

// the key columns of a page and its precomputed raw hashes (null without a hash channel): what the group-by, join and set kernels take
struct KeyInputs {
    std::vector<const DeviceColumn *> keys;
    const int64_t *hashes;
};
KeyInputs key_inputs(const DevicePage &in, const std::vector<int32_t> &channels, int32_t hash_channel)
{
    KeyInputs k{{}, hash_channel >= 0 ? (const int64_t *)in.cols[(size_t)hash_channel].values : nullptr};
    for (int32_t ch : channels) k.keys.push_back(&in.cols[(size_t)ch]);
    return k;
}
}  // namespace

template <class Config, class Op>
SimpleOperatorFactory<Config, Op>::SimpleOperatorFactory(Context *ctx, int32_t operator_id, Config cfg) : ctx_(ctx), operator_id_(operator_id), cfg_(std::move(cfg))
{
    validate(ctx_, cfg_);
}

template <class Config, class Op> std::unique_ptr<Operator> SimpleOperatorFactory<Config, Op>::create_operator()
{
    check_open();
    return std::make_unique<Op>(ctx_, operator_id_, cfg_);
}

template <class Config, class Op> std::unique_ptr<OperatorFactory> SimpleOperatorFactory<Config, Op>::duplicate()
{
    auto f = std::make_unique<SimpleOperatorFactory>(*this);   // (the config is not validated again)
    f->closed_ = false;
    return f;
}

// The protocol of an operator that turns one input page into at most one output page (WorkProcessorOperatorAdapter.java:138-216): input is
// taken while no output is pending, finish() ends it once the pending page is gone.  A subclass says in emit() what a page becomes
// (it sets pending_, or leaves it empty for a page without output rows) and, where its protocol differs, overrides ready() and the
// state queries.
class PageOperator : public Operator {
public:
    using Operator::Operator;
    bool needs_input() override { return !finishing_ && !pending_; }
    void add_input(const tgpu_page *page) override
    {
        ready();
        emit(ingest_page(ctx_, page));
    }
    // a page of this library: channels that pass through share its (reference counted) buffers
    void add_input_owned(const DevicePage &page) override
    {
        ready();
        emit(DevicePage(page));
    }
    std::unique_ptr<OutputPage> get_output() override { return std::move(pending_); }
    void finish() override { finishing_ = true; }
    bool is_finished() override { return finishing_ && !pending_; }

protected:
    virtual void ready()
    {
        TG_CHECK_STATE(!finishing_, "Operator is already finishing");
        TG_CHECK_STATE(!pending_, "Operator still has pending output");
    }
    virtual void emit(DevicePage in) = 0;

    std::unique_ptr<OutputPage> pending_;
    bool finishing_ = false;
};

// =====================================================================================================================
// FilterAndProjectOperator: WorkProcessorOperatorAdapter protocol (M/operator/WorkProcessorOperatorAdapter.java:138-216)
// around PageProcessor (M/operator/FilterAndProjectOperator.java:56-64).  One output page per input page that selects
// at least one row; MergePages (M/operator/project/MergePages.java) is not applied (page boundaries are not part of the
// operator's contract: the reference's tests compare rows, T/operator/OperatorAssertion.java).
// =====================================================================================================================
namespace {
// dictionary-aware selection: row r is selected iff the verdict of its dictionary entry is a non-null true
__global__ void __launch_bounds__(256) dict_select_kernel(const uint8_t *verdict, const uint8_t *verdict_nulls, const int32_t *ids, int64_t n, int32_t *flags)
{
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256) {
        const int32_t e = ids[r];
        flags[r] = (verdict[e] != 0 && !(verdict_nulls && verdict_nulls[e])) ? 1 : 0;
    }
}
__global__ void __launch_bounds__(256) dict_compact_kernel(const int32_t *flags, const int32_t *rank, const int32_t *ids, int64_t n, int32_t *positions, int32_t *sel_ids)
{
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256)
        if (flags[r]) {
            positions[rank[r]] = (int32_t)r;
            sel_ids[rank[r]] = ids[r];
        }
}
}  // namespace

class FilterAndProjectOperator : public PageOperator {
public:
    FilterAndProjectOperator(Context *ctx, int32_t id, const FilterAndProjectConfig &cfg) : PageOperator(ctx, id), processor_(cfg.processor) {}

    void add_input(const tgpu_page *page) override
    {
        ready();
        if (try_dictionary(page)) return;
        emit(ingest_page(ctx_, page));
    }

    // Dictionary-aware processing (M/operator/project/DictionaryAwarePageFilter.java:56-110, DictionaryAwarePageProjection.java:60-160,
    // selected by PageFunctionCompiler.java:176-212 for deterministic single-channel expressions): when every computed expression reads
    // the same channel and that channel arrives as a DictionaryBlock or RunLengthEncodedBlock, the filter and the projections are
    // evaluated once per dictionary entry (once in all for RLE) and mapped through the ids -- same rows, same values as the flat path.
    // An entry that raises (overflow, division by zero) may belong to no selected row: like the reference (which catches and
    // re-processes the block the normal way, DictionaryAwarePageProjection.java:139-152) the page then takes the flat path.
    bool try_dictionary(const tgpu_page *page)
    {
        const int c = processor_->single_input_channel();
        if (c < 0 || page == nullptr || c >= page->channel_count || getenv("TGPU_DISABLE_DICTIONARY_AWARE")) return false;
        const tgpu_block &blk = page->blocks[c];
        if (blk.encoding == TGPU_FLAT || blk.dictionary == nullptr || blk.dictionary->encoding != TGPU_FLAT) return false;
        const int64_t n = page->position_count;
        if (n == 0 || (int64_t)blk.dictionary->position_count * 2 > n) return false;   // a dictionary about as long as the page: nothing to gain
        for (int32_t ch = 0; ch < page->channel_count; ch++) TG_CHECK_ARG(page->blocks[ch].position_count == page->position_count, "block position count differs from the page's");
        DeviceColumn dict;
        BufferPtr ids;
        ingest_dictionary(ctx_, &blk, dict, ids);
        DevicePage per_entry;
        try {
            ProfileScope ps(ctx_, "dictionary_entries");
            processor_->process_dictionary(ctx_, dict, per_entry);
        }
        catch (const Error &e) {
            if (e.code == TGPU_ERR_NUMERIC_VALUE_OUT_OF_RANGE || e.code == TGPU_ERR_DIVISION_BY_ZERO || e.code == TGPU_ERR_INVALID_CAST_ARGUMENT) return false;
            throw;
        }
        dictionary_pages_++;
        const bool has_filter = processor_->has_filter();
        const int first_slot = has_filter ? 1 : 0;
        int64_t n_sel = n;
        BufferPtr positions, sel_ids = ids;
        if (has_filter) {
            const DeviceColumn &verdict = per_entry.cols[0];
            BufferPtr flags = ctx_->alloc((size_t)n * 4), rank = ctx_->alloc((size_t)n * 4), total = ctx_->alloc(8);
            const int g = grid_for(ctx_, n);
            ProfileScope ps(ctx_, "dictionary_select");
            dict_select_kernel<<<g, 256, 0, ctx_->stream()>>>((const uint8_t *)verdict.values, verdict.nulls, ids->as<int32_t>(), n, flags->as<int32_t>());
            k::exclusive_scan_i32(ctx_, flags->as<int32_t>(), rank->as<int32_t>(), n, total->as<int64_t>());
            n_sel = ctx_->read_scalar(total->as<int64_t>());
            if (n_sel == 0) return true;   // no output page (PageProcessor.java:122-124)
            if (n_sel < n) {
                positions = ctx_->alloc((size_t)n_sel * 4);
                sel_ids = ctx_->alloc((size_t)n_sel * 4);
                dict_compact_kernel<<<g, 256, 0, ctx_->stream()>>>(flags->as<int32_t>(), rank->as<int32_t>(), ids->as<int32_t>(), n, positions->as<int32_t>(), sel_ids->as<int32_t>());
                check_launch("dict_compact");
            }
        }
        DevicePage out;
        out.n = n_sel;
        std::vector<DeviceColumn> flat((size_t)page->channel_count);   // other channels are ingested only when a projection passes them through
        std::vector<bool> have((size_t)page->channel_count, false);
        for (int p = 0; p < processor_->projection_count(); p++) {
            const int ident = processor_->identity_channel(p);
            if (ident < 0) out.cols.push_back(k::gather_column(ctx_, per_entry.cols[(size_t)(first_slot + processor_->computed_slot(p))], sel_ids->as<int32_t>(), n_sel, false));
            else if (ident == c) out.cols.push_back(k::gather_column(ctx_, dict, sel_ids->as<int32_t>(), n_sel, false));
            else {
                if (!have[(size_t)ident]) {
                    flat[(size_t)ident] = ingest_block(ctx_, &page->blocks[ident]);
                    have[(size_t)ident] = true;
                }
                if (positions) out.cols.push_back(k::gather_column(ctx_, flat[(size_t)ident], positions->as<int32_t>(), n_sel, false));
                else out.cols.push_back(flat[(size_t)ident]);
            }
        }
        ctx_->sync();   // host blocks ingested above are only valid during the call
        own_borrowed_columns(ctx_, out);
        pending_ = wrap(std::move(out));
        return true;
    }
    int64_t dictionary_pages() const { return dictionary_pages_; }
    int64_t memory_bytes() override { return pending_ ? pending_->page.size_in_bytes() : 0; }

private:
    void emit(DevicePage in) override
    {
        DevicePage out;
        if (!processor_->process(ctx_, in, out)) return;
        // An identity projection (InputPageProjection) may pass an input block through unchanged.  The output page must outlive
        // the call and the input page (tgpu.h ownership rule): a passed-through block that borrows the caller's device memory
        // is copied; one that came with owners (host ingest, add_input_owned) keeps them alive through its BufferPtrs.
        own_borrowed_columns(ctx_, out);
        pending_ = wrap(std::move(out));
    }

    std::shared_ptr<PageProcessorGpu> processor_;
    int64_t dictionary_pages_ = 0;   // input pages that took the dictionary-aware path
};
static void validate(Context *, const FilterAndProjectConfig &) {}   // (PageProcessorGpu::shared has checked the spec)

// how many input pages of a FilterAndProjectOperator were processed once per dictionary entry (tests, stats)
int64_t filter_project_dictionary_pages(Operator *op)
{
    auto *p = dynamic_cast<FilterAndProjectOperator *>(op);
    TG_CHECK_ARG(p != nullptr, "not a FilterAndProjectOperator");
    return p->dictionary_pages();
}

// =====================================================================================================================
// ScanFilterAndProjectOperator, page-source flavour (M/operator/ScanFilterAndProjectOperator.java:232-287,354-397): a source operator.
// addSplit hands it the split's ConnectorPageSource; getOutput pulls the next page (ConnectorPageSourceToPages.process :368-397:
// finished / blocked / null page = yield) and runs the page processor over it.  LazyBlocks are loaded on demand, in the order the
// reference's PageProcessor touches them (PageProcessor.java:111-137): the channels the filter reads first; the channels only the
// projections read when -- and only when -- the filter selected a row (T/operator/project/TestPageProcessor.java:156-184,219-253).
// =====================================================================================================================
class ScanFilterAndProjectOperator : public Operator {
public:
    ScanFilterAndProjectOperator(Context *ctx, int32_t id, const ScanFilterAndProjectConfig &cfg) : Operator(ctx, id), types_(cfg.types), processor_(cfg.processor) {}
    ~ScanFilterAndProjectOperator() override { close(); }

    bool needs_input() override { return false; }                                                                    // :188-191
    void add_input(const tgpu_page *) override { fail(TGPU_ERR_NOT_SUPPORTED, "ScanFilterAndProjectOperator is a source operator"); }

    void add_page_source(const tgpu_page_source *src)
    {
        TG_CHECK_ARG(src && src->get_next_page && src->is_finished, "page source callbacks are null");
        TG_CHECK_STATE(!no_more_splits_ && !closed_, "no more splits can be added");
        TG_CHECK_STATE(!have_source_, "Table scan split already set");                                               // :235
        source_ = *src;
        have_source_ = true;
    }
    void no_more_splits() { no_more_splits_ = true; }

    // waiting for a split, or for the page source (:214-230)
    bool is_blocked() override
    {
        if (closed_ || finishing_) return false;
        if (!have_source_) return !no_more_splits_;
        return source_.is_blocked && source_.is_blocked(source_.user) == 1;
    }

    std::unique_ptr<OutputPage> get_output() override
    {
        if (closed_ || finishing_ || !have_source_ || is_blocked()) return nullptr;
        if (source_.is_finished(source_.user) == 1) {
            release_source();
            return nullptr;
        }
        tgpu_page page{};
        const int32_t rc = source_.get_next_page(source_.user, &page);
        if (rc < 0) fail(TGPU_ERR_INTERNAL, "the page source failed");
        if (rc == 0) {                                                                                             // null page: finished or yield (:381-388)
            if (source_.is_finished(source_.user) == 1) release_source();
            return nullptr;
        }
        processed_positions_ += page.position_count;
        DevicePage out;
        if (!process(page, out)) return nullptr;
        own_borrowed_columns(ctx_, out);
        return wrap(std::move(out));
    }

    void finish() override
    {
        finishing_ = true;
        release_source();
    }
    bool is_finished() override { return closed_ || finishing_ || (no_more_splits_ && !have_source_); }
    void close() override
    {
        release_source();
        closed_ = true;
    }
    void stats(int64_t *positions, int64_t *loaded, int64_t *skipped) const
    {
        *positions = processed_positions_;
        *loaded = lazy_loaded_;
        *skipped = lazy_skipped_;
    }

private:
    void release_source()
    {
        if (have_source_ && source_.close) source_.close(source_.user);
        have_source_ = false;
    }

    DeviceColumn load_channel(const tgpu_page &page, int ch)
    {
        const tgpu_block &b = page.blocks[ch];
        if (b.encoding != TGPU_LAZY) return ingest_block(ctx_, &b);
        TG_CHECK_ARG(source_.load_block != nullptr, "the page has lazy blocks but the page source has no load_block");
        tgpu_block loaded{};
        if (source_.load_block(source_.user, ch, &loaded) < 0) fail(TGPU_ERR_INTERNAL, "the page source failed to load a lazy block");
        TG_CHECK_ARG(loaded.encoding != TGPU_LAZY && loaded.position_count == page.position_count && loaded.type == types_[(size_t)ch], "bad loaded block");
        lazy_loaded_++;
        return ingest_block(ctx_, &loaded);
    }

    bool process(const tgpu_page &page, DevicePage &out)
    {
        TG_CHECK_ARG(page.channel_count == (int32_t)types_.size(), "page channel count differs from the scan's types");
        const int64_t n = page.position_count;
        if (n == 0) return false;
        int lazy = 0;
        for (int32_t ch = 0; ch < page.channel_count; ch++) {
            TG_CHECK_ARG(page.blocks[ch].position_count == page.position_count && page.blocks[ch].type == types_[(size_t)ch], "bad block in the scanned page");
            lazy += page.blocks[ch].encoding == TGPU_LAZY ? 1 : 0;
        }
        DevicePage in;
        in.n = n;
        in.cols.resize(types_.size());
        std::vector<bool> have(types_.size(), false);
        for (size_t i = 0; i < types_.size(); i++) {   // placeholders: a channel no expression reads is never dereferenced
            in.cols[i].type = types_[i];
            in.cols[i].n = n;
        }
        auto need = [&](int ch) {
            if (have[(size_t)ch]) return;
            in.cols[(size_t)ch] = load_channel(page, ch);
            have[(size_t)ch] = true;
        };
        for (int ch : processor_->filter_channels()) need(ch);
        bool projection_only_lazy = false;
        for (int ch : processor_->projection_channels()) projection_only_lazy = projection_only_lazy || (!have[(size_t)ch] && page.blocks[ch].encoding == TGPU_LAZY);
        if (processor_->has_filter() && projection_only_lazy) {
            // would any row survive?  Only then are the projections' lazy blocks loaded (the filter runs again with them in place)
            DevicePage none;
            if (!processor_->filter_only()->process(ctx_, in, none)) {
                for (int ch : processor_->projection_channels())
                    if (!have[(size_t)ch] && page.blocks[ch].encoding == TGPU_LAZY) lazy_skipped_++;
                count_unread(page, have, lazy);
                return false;
            }
        }
        for (int ch : processor_->projection_channels()) need(ch);
        count_unread(page, have, lazy);
        ctx_->sync();   // the source's arrays are valid until its next call; the uploads have consumed them now
        return processor_->process(ctx_, in, out);
    }

    void count_unread(const tgpu_page &page, const std::vector<bool> &have, int lazy)
    {
        if (!lazy) return;
        const std::vector<int> &pc = processor_->projection_channels();
        for (int32_t ch = 0; ch < page.channel_count; ch++)   // lazy channels nobody reads at all
            if (page.blocks[ch].encoding == TGPU_LAZY && !have[(size_t)ch] && std::find(pc.begin(), pc.end(), (int)ch) == pc.end()) lazy_skipped_++;
    }

    std::vector<int32_t> types_;
    std::shared_ptr<PageProcessorGpu> processor_;
    tgpu_page_source source_{};
    bool have_source_ = false, no_more_splits_ = false, finishing_ = false, closed_ = false;
    int64_t processed_positions_ = 0, lazy_loaded_ = 0, lazy_skipped_ = 0;
};

static void validate(Context *, const ScanFilterAndProjectConfig &) {}

static ScanFilterAndProjectOperator *as_scan(Operator *op)
{
    auto *p = dynamic_cast<ScanFilterAndProjectOperator *>(op);
    TG_CHECK_ARG(p != nullptr, "not a ScanFilterAndProjectOperator");
    return p;
}
void scan_add_page_source(Operator *op, const tgpu_page_source *source) { as_scan(op)->add_page_source(source); }
void scan_no_more_splits(Operator *op) { as_scan(op)->no_more_splits(); }
void scan_stats(Operator *op, int64_t *processed_positions, int64_t *lazy_loaded, int64_t *lazy_skipped) { as_scan(op)->stats(processed_positions, lazy_loaded, lazy_skipped); }

// =====================================================================================================================
// HashAggregationOperator + InMemoryHashAggregationBuilder
// =====================================================================================================================
class HashAggregationOperator : public Operator {
public:
    HashAggregationOperator(Context *ctx, int32_t id, const HashAggregationConfig &cfg) : Operator(ctx, id), cfg_(cfg)
    {
        TG_CHECK_ARG(cfg_.group_by_types.size() == cfg_.group_by_channels.size(), "group-by types and channels differ in length");
        TG_CHECK_ARG(cfg_.step >= TGPU_STEP_SINGLE && cfg_.step <= TGPU_STEP_FINAL, "unknown aggregation step");
    }

    // HashAggregationOperator.java:367-378
    bool needs_input() override
    {
        if (finishing_) return false;
        if (builder_full()) return false;
        return true;
    }

    // :381-440 -> InMemoryHashAggregationBuilder.processPage (builder/InMemoryHashAggregationBuilder.java:139-155)
    void add_input(const tgpu_page *page) override
    {
        begin_input();
        DevicePage in = ingest_page(ctx_, page);
        process_page(in);
    }

protected:
    void begin_input()
    {
        TG_CHECK_STATE(!finishing_, "Operator is already finishing");
        TG_CHECK_STATE(!builder_full(), "Aggregation buffer is full");
        input_processed_ = true;
        ensure_builder();
    }

    // ---- small input pages are coalesced in HBM before they meet the group-by table ----------------------------------------------------------
    // A join's output pages are a fraction of its probe pages (TPCH Q3: 5 K rows out of a 2^20-row probe page), and every page costs the
    // group-by its insert / rank / publish protocol: launches and a read-back, whatever its size.  What the reference solves with MergePages
    // in front of its operators (M/operator/project/MergePages.java) happens inside the operator here: pages below kCoalesceBelowRows rows
    // are appended to a device column store (ONE launch per page, no read-back: fixed-width channels only) and processed as one page once
    // kCoalesceFlushRows rows are there -- or when the operator's state is needed (finish, output, revoke).  Rows keep their order, so
    // group ids and row-order sums are those of the unmerged stream.  Not for PARTIAL steps (their memory limit is checked per page).
    static constexpr int64_t kCoalesceBelowRows = 1 << 20, kCoalesceFlushRows = 1 << 22;
    bool coalesce(const DevicePage &in)
    {
        if (!gbh_ || cfg_.step == TGPU_STEP_PARTIAL || getenv("TGPU_DISABLE_COALESCE")) return false;
        const bool small = in.n < kCoalesceBelowRows;
        if (!small) {
            flush_coalesced();   // (order: what was buffered came first)
            return false;
        }
        for (const DeviceColumn &c : in.cols)
            if (c.type == TGPU_VARCHAR) {
                flush_coalesced();
                return false;
            }
        if (!pending_pages_) {
            std::vector<int32_t> types;
            for (const DeviceColumn &c : in.cols) types.push_back(c.type);
            pending_pages_ = std::make_unique<PagesIndexGpu>(ctx_, types);
        }
        TG_CHECK_ARG(pending_pages_->types().size() == in.cols.size(), "page channel count changed between pages");
        static const std::vector<std::array<int32_t, 2>> no_ends(64, {0, 0});
        pending_pages_->add_page(in, &no_ends);
        if (pending_pages_->position_count() >= kCoalesceFlushRows) flush_coalesced();
        return true;
    }
    void flush_coalesced()
    {
        if (!pending_pages_ || pending_pages_->position_count() == 0) return;
        std::unique_ptr<PagesIndexGpu> store = std::move(pending_pages_);
        DevicePage merged;
        merged.n = store->position_count();
        for (int ch = 0; ch < (int)store->types().size(); ch++) merged.cols.push_back(store->column(ch));
        process_page_now(merged);
    }

    void process_page(const DevicePage &in)
    {
        if (in.n == 0) return;
        if (coalesce(in)) return;
        process_page_now(in);
    }

    void process_page_now(const DevicePage &in)
    {
        const int32_t *gids = nullptr;
        BufferPtr gid_buf;
        bool ascending = false;
        if (gbh_) {
            for (int32_t ch : cfg_.group_by_channels) TG_CHECK_ARG(ch >= 0 && ch < (int)in.cols.size(), "group-by channel out of range");
            if (cfg_.hash_channel >= 0)
                TG_CHECK_ARG(cfg_.hash_channel < (int)in.cols.size() && in.cols[(size_t)cfg_.hash_channel].type == TGPU_BIGINT, "bad hash channel");
            const auto [keys, hashes] = key_inputs(in, cfg_.group_by_channels, cfg_.hash_channel);
            gid_buf = ctx_->alloc((size_t)in.n * 4);
            // a page that takes the group-by's run route brings along what the accumulate side would otherwise read back for itself: that its
            // ids ascend (no sort check) and, for the page that crosses the mode prefix, the number of groups in front of the mark
            GbhRunInfo run;
            run.prefix_rows = prefix_rows_in(in.n);
            gbh_->get_group_ids(keys, hashes, in.n, gid_buf->as<int32_t>(), nullptr, false, nullptr, nullptr, nullptr, nullptr, &run);
            gids = gid_buf->as<int32_t>();
            ascending = run.by_runs;
            if (hold_back(in, gid_buf, nullptr, /*lowcard_max_groups=*/0, &run)) return;
        }
        accumulate_page(gids, in, ascending);
    }

    void accumulate_page(const int32_t *gids, const DevicePage &in, bool gids_ascending = false)
    {
        const int64_t groups = gbh_ ? gbh_->group_count() : 1;
        if (cfg_.step == TGPU_STEP_FINAL) accs_->add_intermediate(gids, in.n, in, groups, gids_ascending);
        else accs_->add_input(gids, in.n, in, groups, gids_ascending);
    }

    // ---- the DOUBLE mode is decided from the first kModePrefixRows rows of the stream, however they are cut into pages (agg.h) ----------------
    // Pages that arrive before that many rows have been seen are kept (an owned copy + their group ids: they are small) and accumulated, in
    // order, once the mode is known; the page that crosses the mark tells how many groups its first rows hold.  Returns true when the page
    // has been kept back.  The group-by table itself always runs at once: group ids do not depend on the mode.
    struct HeldPage {
        DevicePage page;
        BufferPtr gids, gids8;
        bool ascending = false;   // the ids came from the group-by's run route
    };
    static int64_t mode_prefix_rows()
    {
        return getenv("TGPU_MODE_PREFIX_ROWS") ? atoll(getenv("TGPU_MODE_PREFIX_ROWS")) : GroupedAccumulators::kModePrefixRows;   // (tests shorten it)
    }
    // how many rows of a page of n rows belong to the mode prefix when the page is the one that crosses the mark (hold_back's m); else 0
    int64_t prefix_rows_in(int64_t n) const
    {
        if (!accs_ || accs_->decided()) return 0;
        const int64_t prefix = mode_prefix_rows();
        return rows_seen_ + n < prefix ? 0 : std::max<int64_t>(prefix - rows_seen_, 1);
    }
    bool hold_back(const DevicePage &in, const BufferPtr &gids, const BufferPtr &gids8, int64_t lowcard_max_groups, const GbhRunInfo *run = nullptr)
    {
        if (accs_->decided()) return false;
        const int64_t prefix = mode_prefix_rows();
        if (rows_seen_ + in.n < prefix) {
            HeldPage h;
            h.page = in;
            resolve_varchar_ends(ctx_, h.page);   // (the fused path leaves the byte ranges of borrowed VARCHAR blocks unread)
            own_borrowed_columns(ctx_, h.page);
            h.gids = gids;
            h.gids8 = gids8;
            h.ascending = run != nullptr && run->by_runs;
            held_.push_back(std::move(h));
            rows_seen_ += in.n;
            groups_in_prefix_ = gbh_->group_count();
            return true;
        }
        const int64_t m = prefix - rows_seen_;
        // a run-route page has the count already: its ids ascend, so the groups among its first m rows are id[m - 1] + 1
        const bool known = run != nullptr && run->by_runs && run->prefix_rows == std::max<int64_t>(m, 1);
        const int64_t here = known ? run->prefix_groups
                                   : GroupedAccumulators::groups_among(ctx_, gids8 ? nullptr : gids->as<int32_t>(), gids8 ? gids8->as<uint8_t>() : nullptr, std::max<int64_t>(m, 1));
        accs_->decide(std::max(groups_in_prefix_, here), lowcard_max_groups);
        rows_seen_ += in.n;
        release_held();
        return false;
    }
    // the stream ended (or its state is needed) before the prefix was full: every row seen so far is the prefix
    void decide_now(int64_t lowcard_max_groups = 0)
    {
        if (!accs_ || accs_->decided() || held_.empty()) return;
        accs_->decide(gbh_ ? gbh_->group_count() : 1, lowcard_max_groups);
        release_held();
    }
    virtual void release_held()
    {
        std::vector<HeldPage> held = std::move(held_);
        held_.clear();
        for (HeldPage &h : held) accumulate_page(h.gids ? h.gids->as<int32_t>() : nullptr, h.page, h.ascending);
    }

public:
    // :470-518
    std::unique_ptr<OutputPage> get_output() override
    {
        if (finished_) return nullptr;
        if (finishing_) flush_coalesced();
        if (finishing_ || builder_full()) decide_now(held_lowcard_max_groups());
        if (finishing_) {
            if (!input_processed_ && cfg_.produce_default_output && cfg_.group_by_types.empty()) {
                // global aggregation without input: one row of default values (count 0, sum NULL) :481-485
                ensure_builder();
            }
            finished_ = true;
            producing_output_ = true;
            if (!runs_.empty()) merge_runs();   // SpillableHashAggregationBuilder.buildResult :193-240
            if (!builder_) return nullptr;
            std::unique_ptr<OutputPage> out = build_result();
            reset_builder();
            return out;
        }
        if (!builder_full()) return nullptr;  // only flush when finishing or full :494-497
        std::unique_ptr<OutputPage> out = build_result();
        reset_builder();
        return out;
    }

    void finish() override { finishing_ = true; }
    bool is_finished() override { return finished_; }
    // SpillableHashAggregationBuilder.updateMemory :117-128: until output is produced the builder's memory is revocable
    int64_t memory_bytes() override { return revocable() ? 0 : builder_bytes(); }
    int64_t revocable_memory_bytes() override { return revocable() ? builder_bytes() : 0; }

    // startMemoryRevoke -> spillToDisk (:160-168, :283-299): the builder's groups leave HBM as one run -- keys, raw hashes and the
    // EXACT accumulator state (GroupedAccumulators::dump), parked in host memory -- and an empty builder takes over.  The reference
    // sorts a run by hash for its merge of bounded memory; here the runs are merged through the group-by table when the output is
    // built (288 GB of HBM: the merge itself is not what memory pressure is about), and the output comes out in raw-hash order like
    // the reference's merged result.
    void start_memory_revoke() override
    {
        if (!revocable() || !builder_) return;
        spill_run();
    }
    void spill_stats(int64_t &spill_count, int64_t &spilled_bytes) override
    {
        spill_count = spill_count_;
        spilled_bytes = spilled_bytes_;
    }

protected:
    int64_t builder_bytes() const
    {
        return (gbh_ ? gbh_->estimated_size() : 0) + (accs_ ? accs_->estimated_size() : 0) + (pending_pages_ ? pending_pages_->estimated_size() : 0);
    }
    bool spillable() const { return cfg_.spill_enabled && (cfg_.step == TGPU_STEP_SINGLE || cfg_.step == TGPU_STEP_FINAL); }   // HashAggregationOperator.java:390
    bool revocable() const { return spillable() && !producing_output_; }
    struct SpilledRun {
        int64_t groups = 0;
        std::vector<HostColumn> keys;   // group-by channels, then the raw hash of every group
        GroupedAccumulators::HostStates states;
    };
    void spill_run()
    {
        flush_coalesced();
        decide_now(held_lowcard_max_groups());
        const int64_t groups = gbh_ ? gbh_->group_count() : (input_processed_ ? 1 : 0);
        if (groups > 0) {
            SpilledRun run;
            run.groups = groups;
            if (gbh_) {
                DevicePage keys = gbh_->key_page(true);
                for (const DeviceColumn &c : keys.cols) run.keys.push_back(download_column(ctx_, c));
            }
            run.states = accs_->dump(groups);
            spill_count_++;
            spilled_bytes_ += run.states.bytes();
            for (const HostColumn &h : run.keys) spilled_bytes_ += h.bytes();
            runs_.push_back(std::move(run));
        }
        reset_builder();   // rebuildHashAggregationBuilder :331-351
    }
    // mergeFromDisk :229-240 (after spilling what is still in memory, like the reference does when memory is short): every run's
    // groups are looked up / inserted in a fresh table, their states added exactly
    void merge_runs()
    {
        if (builder_) spill_run();
        ensure_builder();
        accs_->set_allow_ordered(false);
        // all runs in many-group (row-order) mode: combined like the reference, one double add per run in spill order; few-group runs keep
        // their exact limb state and merge exactly (bit-identical with and without spills)
        bool all_ordered = !runs_.empty();
        for (const SpilledRun &run : runs_) {
            bool ordered = false;
            for (const auto &a : run.states.aggs) ordered = ordered || !a.dsum.empty();
            bool has_double = false;
            for (const auto &sp : cfg_.aggs) has_double = has_double || sp.function == TGPU_AGG_SUM_DOUBLE || sp.function == TGPU_AGG_AVG_DOUBLE || sp.function == TGPU_AGG_AVG_BIGINT;
            all_ordered = all_ordered && (ordered || !has_double);
        }
        accs_->set_combine_ordered(all_ordered);
        for (const SpilledRun &run : runs_) {
            BufferPtr gid_buf;
            const int32_t *gids = nullptr;
            if (gbh_) {
                std::vector<DeviceColumn> cols;
                for (const HostColumn &h : run.keys) cols.push_back(upload_column(ctx_, h));
                std::vector<const DeviceColumn *> keys;
                for (size_t i = 0; i + 1 < cols.size(); i++) keys.push_back(&cols[i]);
                const int64_t *hashes = cfg_.hash_channel >= 0 ? (const int64_t *)cols.back().values : nullptr;
                gid_buf = ctx_->alloc((size_t)run.groups * 4);
                gbh_->get_group_ids(keys, hashes, run.groups, gid_buf->as<int32_t>());
                gids = gid_buf->as<int32_t>();
            }
            accs_->merge(gids, run.states, gbh_ ? gbh_->group_count() : 1);
        }
        runs_.clear();
        hash_sorted_output_ = gbh_ != nullptr;
    }

    void ensure_builder()
    {
        if (builder_) return;
        if (!cfg_.group_by_types.empty())
            gbh_ = std::make_unique<GroupByHashGpu>(ctx_, cfg_.group_by_types, cfg_.hash_channel >= 0, cfg_.expected_groups, allow_integer_table());
        accs_ = std::make_unique<GroupedAccumulators>(ctx_, cfg_.aggs, cfg_.step);
        accs_->set_allow_ordered(allow_ordered_accumulation());
        accs_->set_force_ordered(ctx_->double_sum_order() == TGPU_SUM_ORDER_JAVA);
        builder_ = true;
    }
    // many groups: rows sorted by group id, one lane per group adds them in row order (agg.h)
    virtual bool allow_ordered_accumulation() const { return true; }
    // the single-integer-key table (groupby_bigint.hip); an operator that brings its own probe kernels needs the generic layout
    virtual bool allow_integer_table() const { return true; }
    void reset_builder()
    {
        gbh_.reset();
        accs_.reset();
        builder_ = false;
        held_.clear();
        rows_seen_ = 0;
        groups_in_prefix_ = 0;
    }
    virtual int64_t held_lowcard_max_groups() const { return 0; }
    // InMemoryHashAggregationBuilder.isFull :208-215: only partial aggregations have a memory limit
    bool builder_full()
    {
        if (!builder_ || cfg_.step != TGPU_STEP_PARTIAL) return false;
        // the limit is on the logical size of the partial state (what the Java builder would hold: 13 B per slot at 0.75
        // fill + keys + accumulator state), not on this implementation's over-provisioned device buffers
        const int64_t groups = gbh_ ? gbh_->group_count() : 1;
        const int64_t per_group = 18 + 9 * (int64_t)cfg_.group_by_types.size() + 16 * (int64_t)cfg_.aggs.size();
        return groups * per_group > cfg_.max_partial_memory;
    }
    // buildResult :244-298: groups in group-id order; keys, [hash], aggregates
    std::unique_ptr<OutputPage> build_result()
    {
        DevicePage out;
        const int64_t groups = gbh_ ? gbh_->group_count() : 1;
        if (gbh_) out = gbh_->key_page(cfg_.hash_channel >= 0);
        out.n = groups;
        accs_->evaluate(groups, out.cols);
        if (groups == 0) return nullptr;
        if (hash_sorted_output_ && groups > 1) {
            // merged runs come out in raw-hash order (MergeHashSort.java:58-101: Long.compare of the hashes; equal hashes keep the
            // order in which the runs brought them)
            DevicePage hp;
            hp.n = groups;
            hp.cols.push_back(gbh_->key_page(true).cols.back());
            int64_t count = 0;
            BufferPtr order = TopNGpu::sorted_positions(ctx_, hp, {0}, {TGPU_SORT_ASC_NULLS_LAST}, groups, count);
            DevicePage sorted;
            sorted.n = groups;
            for (const DeviceColumn &c : out.cols) sorted.cols.push_back(k::gather_column(ctx_, c, order->as<int32_t>(), groups, false));
            out = std::move(sorted);
        }
        return wrap(std::move(out));
    }

    HashAggregationConfig cfg_;
    std::unique_ptr<GroupByHashGpu> gbh_;
    std::unique_ptr<GroupedAccumulators> accs_;
    std::vector<HeldPage> held_;
    std::unique_ptr<PagesIndexGpu> pending_pages_;
    int64_t rows_seen_ = 0, groups_in_prefix_ = 0;
    bool builder_ = false, finishing_ = false, finished_ = false, input_processed_ = false;
    std::vector<SpilledRun> runs_;
    bool producing_output_ = false, hash_sorted_output_ = false;
    int64_t spill_count_ = 0, spilled_bytes_ = 0;
};

static void validate(Context *, const HashAggregationConfig &cfg)
{
    TG_CHECK_ARG(cfg.group_by_types.size() == cfg.group_by_channels.size(), "group-by types and channels differ in length");
    TG_CHECK_ARG((int)cfg.group_by_types.size() <= kMaxKeyChannels, "at most 8 group-by channels");
    TG_CHECK_ARG((int)cfg.aggs.size() <= kMaxAggs, "at most 16 aggregates");
    TG_CHECK_ARG(cfg.expected_groups > 0, "expectedGroups must be positive");
    for (auto &a : cfg.aggs) TG_CHECK_ARG(agg_function_known(a.function), "unknown aggregate function");
}

// =====================================================================================================================
// StreamingAggregationOperator (M/operator/StreamingAggregationOperator.java:216-347): the input arrives grouped on the keys, a group is a
// maximal run of consecutive rows whose key rows are not distinct (rowNotDistinctFromRow), across any number of pages.
//   per page   sagg_detect numbers the page's runs 0.. (id 0 = the group the previous page left open, if row 0 continues it -- or a
//              group without a row here, if it does not), the accumulators -- ORDERED from the start -- add the rows in row order from
//              those ascending ids, groups [0, g - 1) are evaluated and leave as one page, group g - 1's state moves to group 0
//              (GroupedAccumulators::carry_last_group) and the page's last row becomes the carried key row (currentGroup, :303).
//   key cells  :283-305,317-324: a group that ends inside the page takes the first row of its segment in this page (row 0 for a group that
//              began earlier); a group flushed by the next page's first row or by finish takes the carried row = the last row of its page.
//   raises     sum(bigint) overflow: the add_input whose page completes the group, or finish for the last group; nothing of that page
//              is emitted.
// Input pages are not coalesced: every page pays its launches and its read-back.
// =====================================================================================================================
class StreamingAggregationOperator : public Operator {
public:
    StreamingAggregationOperator(Context *ctx, int32_t id, const StreamingAggregationConfig &cfg)
        : Operator(ctx, id), cfg_(cfg), accs_(ctx, cfg.aggs, cfg.step, /*ordered_from_start=*/true)
    {
    }

    bool needs_input() override { return !finishing_ && output_.empty(); }   // :237-242: queued output goes out before the next page comes in
    void add_input(const tgpu_page *page) override
    {
        ready();
        process(ingest_page(ctx_, page));
    }
    void add_input_owned(const DevicePage &page) override
    {
        ready();
        process(page);
    }
    std::unique_ptr<OutputPage> get_output() override
    {
        if (output_.empty()) return nullptr;
        std::unique_ptr<OutputPage> out = std::move(output_.front());
        output_.pop_front();
        return out;
    }
    // :219-235: the open group is evaluated and flushed
    void finish() override
    {
        if (finishing_) return;
        finishing_ = true;
        if (carry_.empty()) return;
        DevicePage out;
        out.n = 1;
        out.cols = std::move(carry_);
        carry_.clear();
        accs_.evaluate(1, out.cols);
        output_.push_back(wrap(std::move(out)));
    }
    bool is_finished() override { return finishing_ && output_.empty(); }
    int64_t memory_bytes() override
    {
        int64_t s = accs_.estimated_size();
        for (const DeviceColumn &c : carry_) s += c.size_in_bytes();
        for (const auto &p : output_) s += p->page.size_in_bytes();
        return s;
    }

private:
    void ready()
    {
        TG_CHECK_STATE(!finishing_, "Operator is already finishing");
        TG_CHECK_STATE(output_.empty(), "Operator still has pending output");
    }

    DeviceColumn gather_keys(const DeviceColumn &src, const int32_t *positions, int64_t rows)
    {
        DeviceColumn c = k::gather_column(ctx_, src, positions, rows, false);
        if (c.type == TGPU_VARCHAR) {   // the gather's offsets start at 0 and end at its byte total
            c.pool_exact = true;
            c.pool_first = 0;
        }
        return c;
    }

    void process(const DevicePage &in)
    {
        check_page_types(in, cfg_.types);
        if (in.n == 0) return;
        std::vector<const DeviceColumn *> keys;
        for (int32_t ch : cfg_.group_by_channels) keys.push_back(&in.cols[(size_t)ch]);
        const SaggGroups det = sagg_detect(ctx_, keys, in.n, carry_.empty() ? nullptr : &carry_);
        const int64_t groups = det.groups();
        const int32_t *gids = det.gids->as<int32_t>();
        if (cfg_.step == TGPU_STEP_FINAL) accs_.add_intermediate(gids, in.n, in, groups, true);
        else accs_.add_input(gids, in.n, in, groups, true);
        const int64_t completed = groups - 1;
        if (completed > 0) {
            // every segment but the last is a completed group and brings its first row; with `shift` the carried group comes in front
            const int64_t from_page = det.segments - 1;
            DevicePage out;
            out.n = completed;
            if (from_page > 0)
                for (const DeviceColumn *kc : keys) out.cols.push_back(gather_keys(*kc, det.starts->as<int32_t>(), from_page));
            if (det.shift && from_page == 0) out.cols = carry_;
            else if (det.shift) {
                PagesIndexGpu both(ctx_, cfg_.group_by_types);
                DevicePage first, rest;
                first.n = 1;
                first.cols = carry_;
                rest.n = from_page;
                rest.cols = std::move(out.cols);
                both.add_page(first);
                both.add_page(rest);
                out.cols.clear();
                for (int c = 0; c < (int)keys.size(); c++) out.cols.push_back(both.column(c));
            }
            accs_.evaluate(completed, out.cols);   // (may raise: nothing of this page has been queued)
            output_.push_back(wrap(std::move(out)));
            accs_.carry_last_group(groups);
        }
        // currentGroup = the page's last row, as an owned one-row page (:303)
        BufferPtr last = ctx_->alloc(4);
        k::fill_i32(ctx_, last->as<int32_t>(), (int32_t)(in.n - 1), 1);
        std::vector<DeviceColumn> carry;
        for (const DeviceColumn *kc : keys) carry.push_back(gather_keys(*kc, last->as<int32_t>(), 1));
        carry_ = std::move(carry);
    }

    StreamingAggregationConfig cfg_;
    GroupedAccumulators accs_;
    std::vector<DeviceColumn> carry_;   // the key cells of the open group's reference row; empty: no group is open
    std::deque<std::unique_ptr<OutputPage>> output_;
    bool finishing_ = false;
};

static void validate(Context *, const StreamingAggregationConfig &cfg)
{
    TG_CHECK_ARG(!cfg.group_by_channels.empty(), "streaming aggregation needs at least one group-by channel (a global aggregation stays with the hash operator)");
    TG_CHECK_ARG((int)cfg.group_by_channels.size() <= kMaxKeyChannels, "at most 8 group-by channels");
    TG_CHECK_ARG(cfg.step >= TGPU_STEP_SINGLE && cfg.step <= TGPU_STEP_FINAL, "unknown aggregation step");
    TG_CHECK_ARG((int)cfg.aggs.size() <= kMaxAggs, "at most 16 aggregates");
    for (int32_t t : cfg.types) TG_CHECK_ARG(valid_type(t), "unknown channel type");
    for (int32_t ch : cfg.group_by_channels) TG_CHECK_ARG(ch >= 0 && ch < (int)cfg.types.size(), "group-by channel out of range");
    for (auto &a : cfg.aggs) {
        TG_CHECK_ARG(agg_function_known(a.function), "unknown aggregate function");
        if (agg_is_varchar_extreme(a.function)) fail(TGPU_ERR_NOT_SUPPORTED, "min / max over VARCHAR is not supported by the streaming aggregation");
        TG_CHECK_ARG(a.function == TGPU_AGG_COUNT_ALL || (a.input_channel >= 0 && a.input_channel < (int)cfg.types.size()), "aggregate input channel out of range");
        // (the source types are known here: min / max over INTEGER / DATE / TIMESTAMP read a channel of that type -- FINAL reads the BIGINT count channel)
        if (agg_own_type(a.function))
            TG_CHECK_ARG(cfg.types[(size_t)a.input_channel] == (cfg.step == TGPU_STEP_FINAL ? TGPU_BIGINT : agg_own_type(a.function)), "aggregate input type mismatch");
        TG_CHECK_ARG(a.mask_channel < (int)cfg.types.size(), "aggregate mask channel out of range");
        if (a.mask_channel >= 0) TG_CHECK_ARG(cfg.types[(size_t)a.mask_channel] == TGPU_BOOLEAN, "aggregate mask channel is not BOOLEAN");
    }
}

// =====================================================================================================================
// HashBuilderOperator (M/operator/HashBuilderOperator.java:155-191 state machine, spill states omitted: the GPU path reports
// its memory as non-revocable and never spills)
// =====================================================================================================================
class HashBuilderOperator : public Operator {
public:
    enum class State { CONSUMING_INPUT, LOOKUP_SOURCE_BUILT, CLOSED };

    HashBuilderOperator(Context *ctx, int32_t id, const HashBuilderConfig &cfg, std::shared_ptr<LookupSourceFactory> bridge, int partition)
        : Operator(ctx, id), cfg_(cfg), bridge_(std::move(bridge)), index_(std::make_shared<PagesIndexGpu>(ctx, cfg.types)), partition_(partition)
    {
    }

    bool needs_input() override { return state_ == State::CONSUMING_INPUT; }

    // :318-350 -> PagesIndex.addPage
    void add_input(const tgpu_page *page) override
    {
        TG_CHECK_STATE(state_ == State::CONSUMING_INPUT, "Operator is already finishing");
        DevicePage in = ingest_page(ctx_, page);
        index_->add_page(in);  // copies: PagesIndex retains the build side for the table's lifetime (PagesIndex.java:221-228)
    }

    std::unique_ptr<OutputPage> get_output() override { return nullptr; }

    // :478-496 finishInput -> buildLookupSource -> lendPartitionLookupSource
    void finish() override
    {
        if (state_ != State::CONSUMING_INPUT) return;
        index_bytes_ = index_->estimated_size();
        bridge_->lend_partition(partition_, index_);   // the last partition to arrive builds the table (lendPartitionLookupSource)
        index_.reset();
        state_ = State::LOOKUP_SOURCE_BUILT;
    }

    // the operator stays alive (blocked) until the probes no longer need the table (:429-470)
    bool is_blocked() override { return state_ == State::LOOKUP_SOURCE_BUILT && !bridge_->destroyed(); }

    bool is_finished() override
    {
        if (state_ == State::LOOKUP_SOURCE_BUILT && bridge_->destroyed()) close();
        return state_ == State::CLOSED;
    }

    int64_t memory_bytes() override
    {
        if (index_) return index_->estimated_size();
        if (state_ == State::CLOSED) return 0;
        std::shared_ptr<LookupSourceGpu> s = bridge_->lookup_source();
        return s && partition_ == 0 ? s->estimated_size() : index_bytes_;   // the merged table is accounted once, on partition 0
    }

    void close() override { state_ = State::CLOSED; }

private:
    HashBuilderConfig cfg_;
    std::shared_ptr<LookupSourceFactory> bridge_;
    std::shared_ptr<PagesIndexGpu> index_;
    int partition_;
    int64_t index_bytes_ = 0;
    State state_ = State::CONSUMING_INPUT;
};

HashBuilderOperatorFactory::HashBuilderOperatorFactory(Context *ctx, int32_t operator_id, HashBuilderConfig cfg, std::shared_ptr<LookupSourceFactory> bridge)
    : ctx_(ctx), operator_id_(operator_id), cfg_(std::move(cfg)), bridge_(std::move(bridge))
{
    const int nt = (int)cfg_.types.size();
    for (int32_t t : cfg_.types) TG_CHECK_ARG(valid_type(t), "unknown type");
    for (int32_t ch : cfg_.output_channels) TG_CHECK_ARG(ch >= 0 && ch < nt, "output channel out of range");
    TG_CHECK_ARG(!cfg_.hash_channels.empty(), "hash join needs at least one join channel");
    for (int32_t ch : cfg_.hash_channels) TG_CHECK_ARG(ch >= 0 && ch < nt, "join channel out of range");
    TG_CHECK_ARG(cfg_.precomputed_hash_channel < nt, "hash channel out of range");
    for (int32_t ch : cfg_.output_channels) bridge_->build_output_types.push_back(cfg_.types[(size_t)ch]);
    bridge_->build_types = cfg_.types;
    TG_CHECK_ARG(cfg_.partition_count >= 1 && cfg_.partition_count <= 1024 && (cfg_.partition_count & (cfg_.partition_count - 1)) == 0,
                 "the build partition count must be a power of two (LocalPartitionGenerator.java:45-52)");
    const HashBuilderConfig config = cfg_;
    Context *c = ctx_;
    bridge_->set_partitioning(cfg_.partition_count, [config, c](std::vector<std::shared_ptr<PagesIndexGpu>> &parts) {
        const HashBuilderConfig &cfg = config;
        std::shared_ptr<PagesIndexGpu> index = parts[0];
        if (parts.size() > 1) {   // concatenation in partition order
            index = std::make_shared<PagesIndexGpu>(c, cfg.types);
            for (auto &part : parts) {
                if (!part || part->position_count() == 0) continue;
                DevicePage pg;
                pg.n = part->position_count();
                for (size_t i = 0; i < cfg.types.size(); i++) pg.cols.push_back(part->column((int)i));
                index->add_page(pg);
                part.reset();   // the partition's own copy goes back to the allocator as soon as it is merged
            }
        }
        auto source = std::make_shared<LookupSourceGpu>(c, index, cfg.hash_channels, cfg.precomputed_hash_channel, cfg.output_channels);
        source->build();
        return source;
    });
}

std::unique_ptr<Operator> HashBuilderOperatorFactory::create_operator()
{
    check_open();
    TG_CHECK_STATE(created_ < cfg_.partition_count, "one build operator per lookup source partition");
    return std::make_unique<HashBuilderOperator>(ctx_, operator_id_, cfg_, bridge_, created_++);
}

// ---- join filter function: the candidate pairs of a probe page, filtered --------------------------------------------------------
namespace {
// pairs are in (probe position, chain) order: count[row] = surviving pairs of the probe row
__global__ void __launch_bounds__(256) jf_count_kernel(const int32_t *probe_idx, int64_t pairs, int32_t *count)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < pairs; i += (int64_t)gridDim.x * 256) atomicAdd(&count[probe_idx[i]], 1);
}
__global__ void __launch_bounds__(256) jf_emit_count_kernel(const int32_t *count, int64_t n, int32_t *emit)
{
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256) emit[r] = count[r] > 0 ? count[r] : 1;
}
// PROBE_OUTER output: every probe row's surviving pairs, or (row, -1) when it has none (LookupJoinOperator.java:354-361)
__global__ void __launch_bounds__(256) jf_outer_rows_kernel(const int32_t *count, const int32_t *offset, int64_t n, int32_t *out_probe, int32_t *out_build)
{
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256)
        if (count[r] == 0) {
            out_probe[offset[r]] = (int32_t)r;
            out_build[offset[r]] = -1;
        }
}
__global__ void __launch_bounds__(256) jf_outer_pairs_kernel(const int32_t *probe_idx, const int32_t *build_idx, int64_t pairs, const int32_t *start, const int32_t *offset,
                                                             int32_t *out_probe, int32_t *out_build)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < pairs; i += (int64_t)gridDim.x * 256) {
        const int32_t r = probe_idx[i];
        const int64_t at = (int64_t)offset[r] + (i - start[r]);   // the pair's rank among its row's survivors: pairs of a row are adjacent
        out_probe[at] = r;
        out_build[at] = build_idx[i];
    }
}
}  // namespace

// JoinHash.getJoinPosition / getNextJoinPosition with a filter function (M/operator/JoinHash.java:82-130): the positions of a key's
// chain are visited newest -> oldest and those the filter rejects are skipped; a PROBE_OUTER row whose every candidate is rejected comes
// out with a null build side.  Here: the key-equal candidate pairs (in that very order) are filtered by a generated kernel
// evaluating the predicate over (build channels gathered at the build position, probe channels gathered at the probe position).
static void apply_join_filter(Context *ctx, LookupSourceGpu &source, const JoinFilter &jf, const DevicePage &in, bool outer, BufferPtr &probe_idx, BufferPtr &build_idx,
                              int64_t &count)
{
    const int nb = (int)jf.build_types.size();
    TG_CHECK_ARG(jf.probe_types.size() == in.cols.size(), "the join filter's probe types differ from the probe page's channels");
    // the channels the predicate reads, compacted: [referenced build channels..., referenced probe channels..., probe index, build index]
    std::vector<tgpu_expr_node> nodes = jf.nodes;
    std::vector<int> remap((size_t)nb + in.cols.size(), -1);
    std::vector<int32_t> types;
    std::vector<int> sources;
    for (auto &nd : nodes)
        if (nd.kind == TGPU_EX_INPUT) {
            TG_CHECK_ARG(nd.op >= 0 && nd.op < (int)remap.size(), "join filter: input channel out of range");
            if (remap[(size_t)nd.op] < 0) {
                remap[(size_t)nd.op] = (int)types.size();
                types.push_back(nd.op < nb ? jf.build_types[(size_t)nd.op] : jf.probe_types[(size_t)(nd.op - nb)]);
                sources.push_back(nd.op);
            }
            nd.op = remap[(size_t)nd.op];
        }
    const int idx_ch = (int)types.size();
    types.push_back(TGPU_INTEGER);
    types.push_back(TGPU_INTEGER);
    tgpu_expr_node pi{}, bi{};
    pi.kind = bi.kind = TGPU_EX_INPUT;
    pi.type = bi.type = TGPU_INTEGER;
    pi.op = idx_ch;
    bi.op = idx_ch + 1;
    nodes.push_back(pi);
    nodes.push_back(bi);
    const int32_t roots[2] = {(int32_t)nodes.size() - 2, (int32_t)nodes.size() - 1};
    tgpu_page_processor_spec spec{nodes.data(), (int32_t)nodes.size(), jf.pool.data(), (int32_t)jf.pool.size(), jf.root, 2, roots};
    std::shared_ptr<PageProcessorGpu> pp = PageProcessorGpu::shared(types, &spec);

    // candidate pairs (inner semantics: the outer rows are added after the filter)
    DevicePage cand;
    cand.n = count;
    for (int src : sources) {
        if (src < nb) cand.cols.push_back(source.gather_index_channel(src, build_idx->as<int32_t>(), count));
        else cand.cols.push_back(k::gather_column(ctx, in.cols[(size_t)(src - nb)], probe_idx->as<int32_t>(), count, false));
    }
    auto idx_col = [&](const BufferPtr &b) {
        DeviceColumn c;
        c.type = TGPU_INTEGER;
        c.n = count;
        c.values_buf = b;
        c.values = b->ptr();
        return c;
    };
    cand.cols.push_back(idx_col(probe_idx));
    cand.cols.push_back(idx_col(build_idx));
    DevicePage kept;
    int64_t survivors = 0;
    if (count > 0 && pp->process(ctx, cand, kept)) {
        survivors = kept.n;
        probe_idx = kept.cols[0].values_buf;
        build_idx = kept.cols[1].values_buf;
    }
    if (!outer) {
        count = survivors;
        return;
    }
    // PROBE_OUTER / FULL_OUTER: a probe row without a surviving candidate is emitted once, build side null, at its place in the order
    const int64_t n = in.n;
    ProfileScope ps(ctx, "join_filter_outer");
    BufferPtr cnt = ctx->alloc_zero((size_t)n * 4), emit = ctx->alloc((size_t)n * 4), start = ctx->alloc((size_t)n * 4), offset = ctx->alloc((size_t)n * 4), total = ctx->alloc(16);
    const int g = grid_for(ctx, n);
    if (survivors > 0) jf_count_kernel<<<g, 256, 0, ctx->stream()>>>(probe_idx->as<int32_t>(), survivors, cnt->as<int32_t>());
    jf_emit_count_kernel<<<g, 256, 0, ctx->stream()>>>(cnt->as<int32_t>(), n, emit->as<int32_t>());
    k::exclusive_scan_i32(ctx, cnt->as<int32_t>(), start->as<int32_t>(), n, total->as<int64_t>());
    k::exclusive_scan_i32(ctx, emit->as<int32_t>(), offset->as<int32_t>(), n, total->as<int64_t>() + 1);
    int64_t totals[2];
    ctx->download(totals, total->ptr(), 16);
    const int64_t out_count = totals[1];
    if (out_count > 0x7fffffffLL) fail(TGPU_ERR_INSUFFICIENT_RESOURCES, "join output of one probe page cannot exceed 2 billion rows");
    BufferPtr op = ctx->alloc((size_t)out_count * 4), ob = ctx->alloc((size_t)out_count * 4);
    jf_outer_rows_kernel<<<g, 256, 0, ctx->stream()>>>(cnt->as<int32_t>(), offset->as<int32_t>(), n, op->as<int32_t>(), ob->as<int32_t>());
    if (survivors > 0)
        jf_outer_pairs_kernel<<<g, 256, 0, ctx->stream()>>>(probe_idx->as<int32_t>(), build_idx->as<int32_t>(), survivors, start->as<int32_t>(), offset->as<int32_t>(),
                                                           op->as<int32_t>(), ob->as<int32_t>());
    check_launch("join_filter_outer");
    probe_idx = op;
    build_idx = ob;
    count = out_count;
}

// PageJoiner.processProbe + LookupJoinPageBuilder.build for one probe page (M/operator/LookupJoinOperator.java:299-347,
// LookupJoinPageBuilder.java:101-131): probe columns by probe index, then the build side's output columns.
// Returns false when the page produces no output row.
static bool probe_page(Context *ctx, LookupSourceGpu &source, const DevicePage &in, const LookupJoinConfig &cfg, DevicePage &out, const JoinFilter *filter = nullptr)
{
    TG_CHECK_ARG(in.cols.size() == cfg.probe_types.size(), "probe page channel count differs from the operator's types");
    if (in.n == 0) return false;
    if (cfg.probe_hash_channel >= 0) TG_CHECK_ARG(in.cols[(size_t)cfg.probe_hash_channel].type == TGPU_BIGINT, "probe hash channel must be BIGINT");
    const auto [keys, hashes] = key_inputs(in, cfg.probe_join_channels, cfg.probe_hash_channel);
    const bool outer = cfg.join_type == TGPU_JOIN_PROBE_OUTER || cfg.join_type == TGPU_JOIN_FULL_OUTER;
    BufferPtr probe_idx, build_idx;
    int64_t count = 0;
    source.probe(keys, hashes, in.n, outer && !filter, probe_idx, build_idx, count);
    if (filter) apply_join_filter(ctx, source, *filter, in, outer, probe_idx, build_idx, count);
    if (count == 0) return false;  // no output page for this probe page (:276-283 pageBuilder.isEmpty)
    if (cfg.join_type == TGPU_JOIN_LOOKUP_OUTER || cfg.join_type == TGPU_JOIN_FULL_OUTER) source.mark_visited(build_idx->as<int32_t>(), count);   // OuterLookupSource.appendTo
    out.n = count;
    ProfileScope ps(ctx, "join_gather");
    for (int32_t ch : cfg.probe_output_channels) out.cols.push_back(k::gather_column(ctx, in.cols[(size_t)ch], probe_idx->as<int32_t>(), count, false));
    const int nb = (int)source.output_channels().size();
    for (int i = 0; i < nb; i++) out.cols.push_back(source.gather_build(i, build_idx->as<int32_t>(), count, outer));
    return true;
}

// =====================================================================================================================
// LookupJoinOperator / PageJoiner (M/operator/LookupJoinOperator.java:208-378)
// =====================================================================================================================
class LookupJoinOperator : public Operator {
public:
    LookupJoinOperator(Context *ctx, int32_t id, const LookupJoinConfig &cfg, std::shared_ptr<LookupSourceFactory> bridge)
        : Operator(ctx, id), cfg_(cfg), bridge_(std::move(bridge))
    {
        bridge_->probe_created();
    }
    ~LookupJoinOperator() override { close(); }

    // blocked on lookupSourceProviderFuture until the build side lends the table (:235-243) -- unless the probe side has ended: input is only
    // taken once the table is there, so an operator that is finishing without it has had no page and finishes without the build side
    // (TestHashJoinOperator.java:1241-1259 testInnerJoinWithBlockingLookupSourceAndEmptyProbe)
    bool is_blocked() override { return !closed_ && !finishing_ && !bridge_->lookup_source(); }
    bool needs_input() override { return !finishing_ && !pending_ && !is_blocked(); }

    void add_input(const tgpu_page *page) override
    {
        TG_CHECK_STATE(!finishing_, "Operator is already finishing");
        TG_CHECK_STATE(!pending_, "Operator still has pending output");
        std::shared_ptr<LookupSourceGpu> source = bridge_->lookup_source();
        TG_CHECK_STATE(source != nullptr, "Lookup source has not been built yet");
        DevicePage in = ingest_page(ctx_, page);
        DevicePage out;
        std::shared_ptr<const JoinFilter> filter = bridge_->join_filter();
        if (probe_page(ctx_, *source, in, cfg_, out, filter.get())) pending_ = wrap(std::move(out));
    }

    std::unique_ptr<OutputPage> get_output() override { return std::move(pending_); }
    void finish() override { finishing_ = true; }
    bool is_finished() override
    {
        bool done = finishing_ && !pending_;
        if (done) close();
        return done;
    }
    int64_t memory_bytes() override { return pending_ ? pending_->page.size_in_bytes() : 0; }
    void close() override
    {
        if (!closed_) {
            closed_ = true;
            bridge_->probe_closed();
        }
    }

private:
    LookupJoinConfig cfg_;
    std::shared_ptr<LookupSourceFactory> bridge_;
    std::unique_ptr<OutputPage> pending_;
    bool finishing_ = false, closed_ = false;
};

LookupJoinOperatorFactory::LookupJoinOperatorFactory(Context *ctx, int32_t operator_id, LookupJoinConfig cfg, std::shared_ptr<LookupSourceFactory> bridge)
    : ctx_(ctx), operator_id_(operator_id), cfg_(std::move(cfg)), bridge_(std::move(bridge))
{
    const int nt = (int)cfg_.probe_types.size();
    for (int32_t t : cfg_.probe_types) TG_CHECK_ARG(valid_type(t), "unknown type");
    TG_CHECK_ARG(!cfg_.probe_join_channels.empty(), "hash join needs at least one join channel");
    for (int32_t ch : cfg_.probe_join_channels) TG_CHECK_ARG(ch >= 0 && ch < nt, "probe join channel out of range");
    for (int32_t ch : cfg_.probe_output_channels) TG_CHECK_ARG(ch >= 0 && ch < nt, "probe output channel out of range");
    TG_CHECK_ARG(cfg_.probe_hash_channel < nt, "probe hash channel out of range");
    TG_CHECK_ARG(cfg_.join_type >= TGPU_JOIN_INNER && cfg_.join_type <= TGPU_JOIN_FULL_OUTER, "unknown join type");
    if (cfg_.join_type == TGPU_JOIN_LOOKUP_OUTER || cfg_.join_type == TGPU_JOIN_FULL_OUTER) bridge_->outer_expected();   // LookupJoinOperatorFactory.java:88-103
    bridge_->probe_factory_created();
}

std::unique_ptr<Operator> LookupJoinOperatorFactory::create_operator()
{
    check_open();
    return std::make_unique<LookupJoinOperator>(ctx_, operator_id_, cfg_, bridge_);
}

std::unique_ptr<OperatorFactory> LookupJoinOperatorFactory::duplicate() { return std::make_unique<LookupJoinOperatorFactory>(ctx_, operator_id_, cfg_, bridge_); }

void LookupJoinOperatorFactory::no_more_operators()
{
    if (closed_) return;
    closed_ = true;
    bridge_->no_more_probes();
}

// =====================================================================================================================
// LookupOuterOperator (M/operator/LookupOuterOperator.java:32-235): once every probe operator of a LOOKUP_OUTER / FULL_OUTER join
// is done (the outer position iterator future, PartitionedLookupSourceFactory.java:259-297), the build rows nobody matched come
// out in build-position order (OuterLookupSource.java:146-190 OuterPositionIterator -- rows with a null key included: they can never
// match), probe-side output channels null (:188-197), build output channels behind them.  One page (the reference cuts it at
// the page builder's size limit).
// =====================================================================================================================
class LookupOuterOperator : public Operator {
public:
    LookupOuterOperator(Context *ctx, int32_t id, const std::vector<int32_t> &probe_output_types, std::shared_ptr<LookupSourceFactory> bridge)
        : Operator(ctx, id), probe_output_types_(probe_output_types), bridge_(std::move(bridge))
    {
    }
    ~LookupOuterOperator() override { close(); }

    bool is_blocked() override { return !closed_ && !(bridge_->probes_finished() && bridge_->lookup_source()); }
    bool needs_input() override { return false; }                                                        // :163-167
    void add_input(const tgpu_page *) override { fail(TGPU_ERR_NOT_SUPPORTED, "LookupOuterOperator takes no input"); }   // :169-173

    std::unique_ptr<OutputPage> get_output() override
    {
        if (closed_ || is_blocked()) return nullptr;
        std::shared_ptr<LookupSourceGpu> source = bridge_->lookup_source();
        BufferPtr positions;
        int64_t count = 0;
        source->unvisited_positions(positions, count);
        std::unique_ptr<OutputPage> out;
        if (count > 0) {
            DevicePage page;
            page.n = count;
            // null probe channels: a one-position dummy column gathered at position -1 (= null) for every output row
            BufferPtr minus_one = ctx_->alloc((size_t)count * 4);
            k::fill_i32(ctx_, minus_one->as<int32_t>(), -1, count);
            for (int32_t t : probe_output_types_) {
                DeviceColumn dummy;
                dummy.type = t;
                dummy.n = 1;
                dummy.values_buf = ctx_->alloc_zero(8);
                dummy.values = dummy.values_buf->ptr();
                if (t == TGPU_VARCHAR) {
                    dummy.offsets_buf = ctx_->alloc_zero(8);
                    dummy.offsets = dummy.offsets_buf->as<int32_t>();
                }
                page.cols.push_back(k::gather_column(ctx_, dummy, minus_one->as<int32_t>(), count, true));
            }
            const int nb = (int)source->output_channels().size();
            for (int i = 0; i < nb; i++) page.cols.push_back(source->gather_build(i, positions->as<int32_t>(), count, false));
            out = wrap(std::move(page));
        }
        close();   // :219-221
        return out;
    }

    void finish() override { close(); }                    // :150-153
    bool is_finished() override { return closed_; }
    void close() override
    {
        if (!closed_) {
            closed_ = true;
            bridge_->outer_done();   // onClose: the build side may release the table now
        }
    }

private:
    std::vector<int32_t> probe_output_types_;
    std::shared_ptr<LookupSourceFactory> bridge_;
    bool closed_ = false;
};

LookupOuterOperatorFactory::LookupOuterOperatorFactory(Context *ctx, int32_t operator_id, std::vector<int32_t> probe_output_types, std::shared_ptr<LookupSourceFactory> bridge)
    : ctx_(ctx), operator_id_(operator_id), probe_output_types_(std::move(probe_output_types)), bridge_(std::move(bridge))
{
    for (int32_t t : probe_output_types_) TG_CHECK_ARG(valid_type(t), "unknown type");
    bridge_->outer_expected();
}

std::unique_ptr<Operator> LookupOuterOperatorFactory::create_operator()
{
    check_open();
    TG_CHECK_STATE(!created_, "Only one outer operator can be created");   // LookupOuterOperator.java:86-90 (one per lifespan)
    created_ = true;
    return std::make_unique<LookupOuterOperator>(ctx_, operator_id_, probe_output_types_, bridge_);
}

// =====================================================================================================================
// FilterAndProject fused into the probe
// =====================================================================================================================
class FusedFilterProjectJoinOperator : public Operator {
public:
    FusedFilterProjectJoinOperator(Context *ctx, int32_t id, const LookupJoinConfig &cfg, std::shared_ptr<LookupSourceFactory> bridge,
                                   std::shared_ptr<PageProcessorGpu> processor, std::shared_ptr<FusedProbeGpu> fused)
        : Operator(ctx, id), cfg_(cfg), bridge_(std::move(bridge)), processor_(std::move(processor)), fused_(std::move(fused))
    {
        bridge_->probe_created();
    }
    ~FusedFilterProjectJoinOperator() override { close(); }

    bool is_blocked() override { return !closed_ && !finishing_ && !bridge_->lookup_source(); }   // (as LookupJoinOperator: a finishing probe never waits)
    bool needs_input() override { return !finishing_ && ready_.empty() && (int)inflight_.size() <= kDepth && !is_blocked(); }

    // Pages of up to kAsyncBelowRows (2^25) rows are probed asynchronously, kDepth pages deep: add_input prepares pass 1 of the new page and -- once
    // kDepth pages are in flight -- pass 2 of the OLDEST one, whose totals reached the host (through its signal slot) while its successor ran,
    // and puts both into ONE launch (FusedProbeGpu::launch_pair: two latency-bound grids side by side); get_output then hands out the oldest
    // page's output.  So a page's output appears kDepth add_inputs later -- or at finish(), or when the driver polls get_output twice without
    // bringing input (a slow source must not keep finished work back).  The Operator contract allows exactly this (getOutput() may return
    // null whenever it likes; Driver.processInternal polls).  It needs the input pages to stay alive in between: library-owned pages (another
    // operator's output, an ingested host page) are kept by reference, borrowed device blocks only qualify under
    // tgpu_context_set_device_input_stable.  An expression error of a page is raised by the call that completes it.
    static constexpr int kDepth = 2;
    static constexpr int64_t kAsyncBelowRows = 1ll << 25;

    void add_input(const tgpu_page *page) override { add_page(page, nullptr); }
    void add_input_owned(const DevicePage &page) override { add_page(nullptr, &page); }   // (keeps the page's buffers: it may stay in flight)

    // Small pages additionally SHARE launches: pages below kBatchBelowRows rows are collected (by reference) until kBatchRows rows or
    // kBatchPages pages have come together and are probed as one sequence of rows -- one launch, one output page, rows in page order (the
    // kernels' multi variant, FusedProbeGpu::begin over a page list).  A launch costs ~15 us of dependent round trips whatever it covers;
    // a 2^20-row page streams in 3.  What is collected goes out like what is in flight: when enough has come together, at finish(), or when
    // the driver polls twice without bringing a page.
    static constexpr int64_t kBatchBelowRows = 1ll << 22, kBatchRows = 1ll << 24;
    static constexpr int kBatchPages = 64;

    void add_page(const tgpu_page *page, const DevicePage *owned)
    {
        TG_CHECK_STATE(!finishing_, "Operator is already finishing");
        TG_CHECK_STATE(ready_.empty() && (int)inflight_.size() <= kDepth, "Operator still has pending output");
        std::shared_ptr<LookupSourceGpu> source = bridge_->lookup_source();
        TG_CHECK_STATE(source != nullptr, "Lookup source has not been built yet");
        DevicePage in = owned ? DevicePage(*owned) : ingest_page(ctx_, page);
        polls_since_input_ = 0;
        if (in.n == 0) return;
        IntTableView tv;
        std::shared_ptr<const JoinFilter> filter = bridge_->join_filter();   // a join filter function runs on the unfused composition
        const bool fused_ok = !filter && fused_->supported() && cfg_.probe_join_channels.size() == 1 && source->int_table(tv) && tv.links == nullptr &&
                              tv.key_type == fused_->projection_types()[(size_t)cfg_.probe_join_channels[0]] && getenv("TGPU_DISABLE_FUSION") == nullptr;
        if (fused_ok) {
            const bool async = in.n <= kAsyncBelowRows && page_is_retained(ctx_, in, owned ? nullptr : page) && getenv("TGPU_DISABLE_ASYNC_JOIN") == nullptr;
            if (!async) {
                flush_batch();
                complete_all();
                InFlight f = describe(source);
                f.pending = fused_->begin(ctx_, in, *source, f.outer, f.need_positions);
                f.pages.push_back(std::move(in));
                inflight_.push_back(std::move(f));
                complete_all();
                return;
            }
            const bool batching = in.n < kBatchBelowRows && getenv("TGPU_DISABLE_PROBE_BATCHING") == nullptr;
            const int64_t tiles = (in.n + batch_tile_rows() - 1) / batch_tile_rows();
            if (!batch_.empty() && (!batching || batch_source_ != source || (batch_tiles_ + tiles) * batch_tile_rows() > FusedProbeGpu::multi_page_row_limit())) flush_batch();
            batch_source_ = source;
            batch_rows_ += in.n;
            batch_tiles_ += tiles;
            batch_.push_back(std::move(in));
            if (!batching || batch_rows_ >= batch_rows_target() || (int)batch_.size() >= kBatchPages) flush_batch();
            return;
        }
        flush_batch();
        complete_all();
        // unfused composition: FilterAndProject, then the probe
        DevicePage mid, out;
        if (!processor_->process(ctx_, in, mid)) return;
        probe_rows_ += mid.n;
        if (probe_page(ctx_, *source, mid, cfg_, out, filter.get())) ready_.push_back(wrap(std::move(out)));
    }

    std::unique_ptr<OutputPage> get_output() override
    {
        // collected / in flight stays that way while the driver keeps bringing pages; a second poll without input in between, or finish(), completes it
        if (ready_.empty() && (!inflight_.empty() || !batch_.empty()) && !finishing_) polls_since_input_++;
        if (ready_.empty() && (finishing_ || polls_since_input_ >= 2)) {
            flush_batch();
            while (ready_.empty() && !inflight_.empty()) complete_oldest(nullptr);
        }
        if (ready_.empty()) return nullptr;
        std::unique_ptr<OutputPage> out = std::move(ready_.front());
        ready_.pop_front();
        return out;
    }
    void finish() override { finishing_ = true; }
    bool is_finished() override
    {
        bool done = finishing_ && ready_.empty() && inflight_.empty() && batch_.empty();
        if (done) close();
        return done;
    }
    int64_t memory_bytes() override
    {
        int64_t b = 0;
        for (const auto &o : ready_) b += o->page.size_in_bytes();
        for (const InFlight &f : inflight_)
            for (const DevicePage &pg : f.pages) b += pg.size_in_bytes();
        for (const DevicePage &pg : batch_) b += pg.size_in_bytes();
        return b;
    }
    int64_t probe_rows() const { return probe_rows_; }
    void close() override
    {
        if (!closed_) {
            closed_ = true;
            for (InFlight &f : inflight_) fused_->cancel(ctx_, f.pending);
            inflight_.clear();
            batch_.clear();
            bridge_->probe_closed();
        }
    }

private:
    struct InFlight {
        std::vector<DevicePage> pages;   // one page, or the pages of a common launch
        std::shared_ptr<FusedProbeGpu::Pending> pending;
        std::shared_ptr<LookupSourceGpu> source;
        std::vector<DeviceColumn> build_cols;
        bool outer = false, track = false, need_positions = false, gather_fused = false;
    };
    static int64_t batch_tile_rows() { return FusedProbeGpu::multi_page_row_limit() / kFjMultiMaxTiles; }
    static int64_t batch_rows_target()
    {
        const char *e = getenv("TGPU_PROBE_BATCH_ROWS");   // (kernel studies)
        return e ? std::max<int64_t>(1, atoll(e)) : kBatchRows;
    }
    InFlight describe(const std::shared_ptr<LookupSourceGpu> &source) const
    {
        InFlight f;
        f.source = source;
        f.outer = cfg_.join_type == TGPU_JOIN_PROBE_OUTER || cfg_.join_type == TGPU_JOIN_FULL_OUTER;
        f.track = cfg_.join_type == TGPU_JOIN_LOOKUP_OUTER || cfg_.join_type == TGPU_JOIN_FULL_OUTER;
        f.need_positions = f.track || !source->output_channels().empty();
        // fixed-width build output channels are gathered by the probe's emit pass itself (no launch of their own)
        const int nb = (int)source->output_channels().size();
        f.gather_fused = nb > 0 && nb <= kFjMaxBuildCols;
        for (int i = 0; i < nb && f.gather_fused; i++) {
            f.build_cols.push_back(source->build_column(i));
            f.gather_fused = f.build_cols.back().type != TGPU_VARCHAR && f.build_cols.back().values != nullptr;
        }
        return f;
    }
    // what has been collected goes into the pipeline: pass 1 prepared, launched together with pass 2 of the oldest launch in flight when
    // kDepth are in flight and the two can pair, else on its own
    void flush_batch()
    {
        if (batch_.empty()) return;
        InFlight f = describe(batch_source_);
        f.pages = std::move(batch_);
        batch_.clear();
        batch_rows_ = batch_tiles_ = 0;
        std::vector<const DevicePage *> list;
        for (const DevicePage &pg : f.pages) list.push_back(&pg);
        f.pending = fused_->begin(ctx_, list, *f.source, f.outer, f.need_positions, /*launch=*/false);
        if (!f.pending) {
            // no signal slot for a launch over several pages (many operators of this context are inside one): page by page, synchronously
            complete_all();
            for (DevicePage &pg : f.pages) {
                InFlight one = describe(f.source);
                one.pending = fused_->begin(ctx_, pg, *f.source, f.outer, f.need_positions);
                one.pages.push_back(std::move(pg));
                inflight_.push_back(std::move(one));
                complete_all();
            }
            return;
        }
        if ((int)inflight_.size() >= kDepth) {
            try {
                complete_oldest(&f.pending);
            } catch (...) {
                fused_->cancel(ctx_, f.pending);
                throw;
            }
        }
        fused_->launch_probe(ctx_, f.pending);   // (no-op when the pair launch carried it)
        inflight_.push_back(std::move(f));
    }
    void complete_all()
    {
        while (!inflight_.empty()) complete_oldest(nullptr);
    }
    // pass 2 of the oldest launch in flight; with `partner` (prepared, not yet launched) in one launch with the partner's pass 1
    void complete_oldest(const std::shared_ptr<FusedProbeGpu::Pending> *partner)
    {
        InFlight f = std::move(inflight_.front());
        inflight_.pop_front();
        std::vector<DeviceColumn> probe_out, build_out;
        BufferPtr build_idx;
        int64_t count = 0, selected = 0;
        fused_->finish(ctx_, f.pending, f.pages[0], probe_out, build_idx, count, selected, f.gather_fused ? &f.build_cols : nullptr, f.gather_fused ? &build_out : nullptr, /*launch=*/false);
        probe_rows_ += selected;
        if (count == 0) return;
        if (partner && fused_->can_pair(f.pending, *partner)) fused_->launch_pair(ctx_, f.pending, *partner);
        else fused_->launch_emit(ctx_, f.pending);
        if (f.track) f.source->mark_visited(build_idx->as<int32_t>(), count);
        DevicePage out;
        out.n = count;
        out.cols = std::move(probe_out);
        if (f.gather_fused) for (DeviceColumn &c : build_out) out.cols.push_back(std::move(c));
        else {
            ProfileScope ps(ctx_, "join_gather");
            const int nb = (int)f.source->output_channels().size();
            for (int i = 0; i < nb; i++) out.cols.push_back(f.source->gather_build(i, build_idx->as<int32_t>(), count, f.outer));
        }
        ready_.push_back(wrap(std::move(out)));
    }

    LookupJoinConfig cfg_;
    std::shared_ptr<LookupSourceFactory> bridge_;
    std::shared_ptr<PageProcessorGpu> processor_;
    std::shared_ptr<FusedProbeGpu> fused_;
    std::deque<InFlight> inflight_;
    std::deque<std::unique_ptr<OutputPage>> ready_;
    std::vector<DevicePage> batch_;   // pages waiting for their common launch
    std::shared_ptr<LookupSourceGpu> batch_source_;
    int64_t batch_rows_ = 0, batch_tiles_ = 0;
    int polls_since_input_ = 0;
    int64_t probe_rows_ = 0;
    bool finishing_ = false, closed_ = false;
};

FusedFilterProjectJoinOperatorFactory::FusedFilterProjectJoinOperatorFactory(Context *ctx, int32_t operator_id, std::vector<int32_t> input_types,
                                                                             const tgpu_page_processor_spec *spec, LookupJoinConfig cfg,
                                                                             std::shared_ptr<LookupSourceFactory> bridge)
    : ctx_(ctx), operator_id_(operator_id), cfg_(std::move(cfg)), bridge_(std::move(bridge))
{
    processor_ = PageProcessorGpu::shared(input_types, spec);
    cfg_.probe_types = processor_->output_types();
    const int nt = (int)cfg_.probe_types.size();
    TG_CHECK_ARG(!cfg_.probe_join_channels.empty(), "hash join needs at least one join channel");
    for (int32_t ch : cfg_.probe_join_channels) TG_CHECK_ARG(ch >= 0 && ch < nt, "probe join channel out of range");
    for (int32_t ch : cfg_.probe_output_channels) TG_CHECK_ARG(ch >= 0 && ch < nt, "probe output channel out of range");
    TG_CHECK_ARG(cfg_.probe_hash_channel < nt, "probe hash channel out of range");
    TG_CHECK_ARG(cfg_.join_type >= TGPU_JOIN_INNER && cfg_.join_type <= TGPU_JOIN_FULL_OUTER, "unknown join type");
    if (cfg_.join_type == TGPU_JOIN_LOOKUP_OUTER || cfg_.join_type == TGPU_JOIN_FULL_OUTER) bridge_->outer_expected();
    fused_ = FusedProbeGpu::shared(input_types, spec, cfg_.probe_join_channels[0], cfg_.probe_output_channels);
    bridge_->probe_factory_created();
}

std::unique_ptr<Operator> FusedFilterProjectJoinOperatorFactory::create_operator()
{
    check_open();
    return std::make_unique<FusedFilterProjectJoinOperator>(ctx_, operator_id_, cfg_, bridge_, processor_, fused_);
}

std::unique_ptr<OperatorFactory> FusedFilterProjectJoinOperatorFactory::duplicate()
{
    auto f = std::unique_ptr<FusedFilterProjectJoinOperatorFactory>(new FusedFilterProjectJoinOperatorFactory(*this));
    f->closed_ = false;
    bridge_->probe_factory_created();
    return f;
}

void FusedFilterProjectJoinOperatorFactory::no_more_operators()
{
    if (closed_) return;
    closed_ = true;
    bridge_->no_more_probes();
}

// =====================================================================================================================
// FilterAndProject fused into the hash aggregation: the filter becomes a row mask in front of the group-by table and the
// aggregates' input projections are evaluated inside the accumulate kernel (jit.h FusedAggGpu); no row is materialised.
// =====================================================================================================================
class FusedFilterProjectAggregationOperator : public HashAggregationOperator {
public:
    FusedFilterProjectAggregationOperator(Context *ctx, int32_t id, const HashAggregationConfig &cfg, std::shared_ptr<PageProcessorGpu> processor,
                                          std::shared_ptr<FusedAggGpu> fused)
        : HashAggregationOperator(ctx, id, cfg), processor_(std::move(processor)), fused_(std::move(fused))
    {
    }

    bool uses_fused_kernels() const { return fused_->supported() && !fused_->key_inputs().empty() && cfg_.step != TGPU_STEP_FINAL && getenv("TGPU_DISABLE_FUSION") == nullptr; }
    bool allow_integer_table() const override { return !uses_fused_kernels(); }

    void add_input(const tgpu_page *page) override { add_page(page, nullptr); }
    // a page of this library keeps its buffers through the DevicePage's owners: it may wait for a common launch or be re-run after the call
    // (the default, a borrowed view of the page, would only be safe under the caller's device_input_stable promise -- which is about the
    // CALLER's memory, not about an output page it releases right after handing it on)
    void add_input_owned(const DevicePage &page) override { add_page(nullptr, &page); }

    void add_page(const tgpu_page *page, const DevicePage *owned)
    {
        confirm_pending(kOnepassDepth - 1);   // (errors and dirty pages of earlier one-pass launches surface here at the latest)
        begin_input();
        const bool fused_ok = gbh_ && uses_fused_kernels();
        // the fused kernels address VARCHAR bytes through the offsets alone: the byte ranges of borrowed device columns stay unread
        DevicePage in = owned ? DevicePage(*owned) : ingest_page(ctx_, page, /*resolve_varchar=*/!fused_ok);
        if (in.n == 0) return;
        const bool keep = page_is_retained(ctx_, in, owned ? nullptr : page);
        if (!fused_ok) {
            drain_onepass();
            // unfused composition: FilterAndProject, then the aggregation
            DevicePage mid;
            if (processor_->process(ctx_, in, mid)) process_page(mid);
            return;
        }
        // A table-sized page does not need two passes either: its first rows go through the insert protocol in three slices -- they bring
        // the groups and decide the DOUBLE mode -- and if the group set has settled by then (it has for the few-group aggregations this path
        // is for) the REST of the page is one one-pass launch: every input byte read once instead of the key columns twice.  The rest is
        // judged like any one-pass launch: a row of an unknown group makes it dirty and it is re-run through the two-launch path.
        if (in.n >= kSplitAboveRows && pending_.empty() && batch_.empty() && clean_streak_ < kOnepassAfter && keep && getenv("TGPU_DISABLE_ONEPASS") == nullptr &&
            getenv("TGPU_DISABLE_SPECULATION") == nullptr && getenv("TGPU_DISABLE_PAGE_SPLIT") == nullptr) {
            static constexpr int64_t kSlices[3] = {1 << 18, 1 << 18, 1 << 20};
            int64_t at = 0;
            for (int64_t len : kSlices) {
                process_fused(slice_of(in, at, len));
                at += len;
            }
            DevicePage rest = slice_of(in, at, in.n - at);
            if (onepass_ready(keep)) {
                batch_rows_ += rest.n;
                batch_.push_back(std::move(rest));
                launch_onepass();
            } else {
                drain_onepass();
                process_fused(rest);
            }
            return;
        }
        if (onepass_ready(keep)) {
            // the operator is blocking (nothing leaves it before finish): small pages are collected, by reference, into one launch
            batch_rows_ += in.n;
            batch_.push_back(std::move(in));
            if (batch_rows_ >= onepass_batch_rows() || (int)batch_.size() >= kOnepassBatchPages) launch_onepass();
            return;
        }
        drain_onepass();
        process_fused(in);
    }

    // a finishing / revoking / closing operator has no page in flight
    void finish() override
    {
        drain_onepass();
        HashAggregationOperator::finish();
    }
    std::unique_ptr<OutputPage> get_output() override
    {
        if (finishing_) drain_onepass();   // (the driver asks after every addInput: a page in flight stays in flight)
        return HashAggregationOperator::get_output();
    }
    void start_memory_revoke() override
    {
        drain_onepass();
        HashAggregationOperator::start_memory_revoke();
    }
    // (the builder's bytes + the library-owned pages this operator keeps alive: collected for a common launch, or launched and not yet confirmed)
    int64_t memory_bytes() override
    {
        int64_t b = HashAggregationOperator::memory_bytes();
        for (const DevicePage &pg : batch_) b += owned_bytes(pg);
        for (const PendingPage &p : pending_)
            for (const DevicePage &pg : p.pages) b += owned_bytes(pg);
        return b;
    }

private:
    // the two-launch path: group probe (insert protocol when a page brings new groups) + accumulate, one read-back per page
    void process_fused(const DevicePage &in)
    {
        // the filter is fused in front of the group-by table (rows it rejects get group id -1), the key code is generated
        // for the key schema, and the raw hash is computed in the kernel (a $hashvalue channel equals it by construction)
        std::vector<const DeviceColumn *> keys;
        for (int raw : fused_->key_inputs()) keys.push_back(&in.cols[(size_t)raw]);
        // few groups: the ids travel as one byte per row between the two fused kernels (int32 only if the table outgrows a byte)
        BufferPtr gids = ctx_->alloc((size_t)in.n * 4), gids8 = ctx_->alloc((size_t)in.n);
        GbhProbeFn probe = [&](const GbhProbeLaunch &l) { fused_->probe_groups(ctx_, in, l); };
        // steady state (every group of the page exists already, few groups): the accumulate launch goes out behind the probe launch,
        // gated on the probe's counters, and runs while the host waits for them (groupby.h GbhSpeculateFn)
        const int64_t groups_before = gbh_->group_count();
        // (while the DOUBLE mode is still open -- the stream's first rows, agg.h kModePrefixRows -- nothing is accumulated behind the probe)
        const bool may_speculate = fused_->can_speculate(groups_before) && !accs_->force_ordered() && accs_->decided() && getenv("TGPU_DISABLE_SPECULATION") == nullptr;
        GbhSpeculateFn speculate = [&](const unsigned long long *counters) {
            fused_->accumulate(ctx_, in, nullptr, gids8->as<uint8_t>(), groups_before, *accs_, counters);
        };
        bool speculated = false;
        const bool compact = gbh_->get_group_ids(keys, nullptr, in.n, gids->as<int32_t>(), nullptr, /*inline_hash=*/true, &probe, gids8->as<uint8_t>(),
                                                 may_speculate ? &speculate : nullptr, &speculated);
        clean_streak_ = speculated ? clean_streak_ + 1 : 0;   // a speculated page met no new group: the group set is settling
        if (speculated) return;
        if (hold_back(in, compact ? BufferPtr() : gids, compact ? gids8 : BufferPtr(), fused_->lowcard_groups())) return;
        fused_->accumulate(ctx_, in, compact ? nullptr : gids->as<int32_t>(), compact ? gids8->as<uint8_t>() : nullptr, gbh_->group_count(), *accs_);
    }
    int64_t held_lowcard_max_groups() const override { return uses_fused_kernels() ? fused_->lowcard_groups() : 0; }
    void release_held() override
    {
        if (!uses_fused_kernels()) {
            HashAggregationOperator::release_held();
            return;
        }
        std::vector<HeldPage> held = std::move(held_);
        held_.clear();
        for (HeldPage &h : held)
            fused_->accumulate(ctx_, h.page, h.gids ? h.gids->as<int32_t>() : nullptr, h.gids8 ? h.gids8->as<uint8_t>() : nullptr, gbh_->group_count(), *accs_);
    }

    // ---- one launch per page, no read-back in front of the next one (FusedAggGpu::onepass) ------------------------------------------------
    // Entered once the group set has settled (kOnepassAfter consecutive pages without a new group, at most 16 groups).  The host reads a
    // page's counters one call LATER (while its successor runs): clean = nothing to do, the successor's launch made the page's totals
    // final; dirty (a row met a group the launch did not know) = the totals were dropped on the device and the page is re-run here through
    // the insert protocol -- possible because the page is still there: library-owned pages (another operator's output, an ingested host
    // page) are kept by reference, borrowed device blocks only qualify under tgpu_context_set_device_input_stable.  Sums are exact
    // (order-independent), so re-running a page after its successors does not change a bit; new groups still get their ids in page order
    // because a successor that met one of them is dirty itself and is re-run after it.  An expression error of page i is raised by the call
    // that confirms it (the next add_input, finish or get_output).
    // Pages below kOnepassBatchRows (2^24) rows wait (by reference) until that many rows or kOnepassBatchPages pages have come together and go out as
    // ONE launch over the list of pages (fq_onepass_multi): a launch costs ~18 us whatever it covers, 1.3 M rows' worth of streaming.  A dirty
    // launch re-runs its pages one by one in page order, an expression error in a launch of several pages likewise (the re-run raises the
    // error of the first failing page, like the reference).
    static constexpr int kOnepassDepth = 2, kOnepassAfter = 2, kOnepassBatchPages = 64;
    static constexpr int64_t kSplitAboveRows = 1ll << 23;   // pages from here on are split into three leading slices + the rest (add_page)
    static int64_t owned_bytes(const DevicePage &pg)
    {
        for (const DeviceColumn &c : pg.cols)
            if (c.n > 0 && !c.values_buf) return 0;   // borrowed device blocks are the embedding's memory, not this operator's
        return pg.size_in_bytes();
    }
    DevicePage slice_of(const DevicePage &in, int64_t at, int64_t len) const
    {
        DevicePage out;
        out.n = len;
        for (const DeviceColumn &c : in.cols) out.cols.push_back(k::region_of(ctx_, c, at, len));   // views: the buffers are shared
        return out;
    }
    static constexpr int64_t kOnepassBatchRows = 1ll << 24;
    static int64_t onepass_batch_rows()
    {
        const char *e = getenv("TGPU_ONEPASS_BATCH_ROWS");
        return e ? std::max<int64_t>(1, atoll(e)) : kOnepassBatchRows;
    }
    struct PendingPage {
        std::vector<DevicePage> pages;
        BufferPtr descriptors;
        unsigned long long *counters;
        Context::AsyncRead read;
        Context::Signal signal;
    };
    bool onepass_ready(bool keep) const   // keep: page_is_retained
    {
        const bool disabled = getenv("TGPU_DISABLE_ONEPASS") != nullptr || getenv("TGPU_DISABLE_SPECULATION") != nullptr;
        return !disabled && clean_streak_ >= kOnepassAfter && fused_->can_onepass(gbh_->group_count()) && !accs_->force_ordered() && accs_->decided() && !accs_->ordered() &&
               keep;
    }
    void launch_onepass()
    {
        if (batch_.empty()) return;
        PendingPage p;
        p.pages = std::move(batch_);
        batch_.clear();
        batch_rows_ = 0;
        p.counters = gbh_->counter_set();
        const unsigned long long *prev = last_onepass_counters_;
        onepass_blocks_ = ctx_->cu_count();   // one workgroup per CU (the lane-private states fill the LDS), one row of pending totals each
        std::vector<const DevicePage *> list;
        for (const DevicePage &pg : p.pages) list.push_back(&pg);
        // the kernel hands its counters to the host itself (a signal slot); with every slot taken they are copied behind it
        p.signal = ctx_->begin_signal();
        try {
            fused_->onepass(ctx_, list, *accs_, gbh_->key_store_view(), gbh_->group_count(), p.counters, prev, onepass_blocks_, p.signal.device, &p.descriptors);
        } catch (...) {
            ctx_->abandon_signal(p.signal);
            // (nothing was launched: the pages go the two-launch way, after whatever is in flight)
            std::vector<DevicePage> pages = std::move(p.pages);
            confirm_pending(0);
            for (const DevicePage &pg : pages) process_fused(pg);
            return;
        }
        if (p.signal.slot < 0) p.read = ctx_->begin_read(p.counters, 64);
        last_onepass_counters_ = p.counters;
        pending_.push_back(std::move(p));
        confirm_pending(kOnepassDepth);
    }
    // confirms launches, oldest first, until at most `keep` are in flight
    void confirm_pending(size_t keep)
    {
        while (pending_.size() > keep) {
            PendingPage p = std::move(pending_.front());
            pending_.pop_front();
            unsigned long long ctr[8] = {};
            if (p.signal.slot >= 0) {
                unsigned long long w[Context::kSignalWords];
                ctx_->finish_signal(p.signal, w);
                ctr[0] = w[0];
                ctr[2] = w[1];
                ctr[7] = w[2];
            } else ctx_->finish_read(p.read, ctr);
            const bool last = pending_.empty();
            const bool dirty = ctr[0] != 0 || ctr[2] != 0 || ctr[7] != ~0ull;
            if (last) {
                // nobody launched behind it: its pending totals are still on the device, and the host decides
                accs_->resolve_pending(onepass_blocks_, !dirty);
                last_onepass_counters_ = nullptr;
            }
            if (p.pages.size() == 1) raise_expression_error(ctr[7]);
            if (dirty) {
                clean_streak_ = 0;
                // (the launches behind it ran against the same group set: each is judged by its own counters)
                for (const DevicePage &pg : p.pages) process_fused(pg);
            }
        }
    }
    // nothing collected, nothing in flight
    void flush_onepass()
    {
        launch_onepass();
        confirm_pending(0);
    }
    void drain_onepass() { flush_onepass(); }

    std::vector<DevicePage> batch_;   // pages waiting for their common launch
    int64_t batch_rows_ = 0;
    std::deque<PendingPage> pending_;
    const unsigned long long *last_onepass_counters_ = nullptr;
    int64_t onepass_blocks_ = 0;
    int clean_streak_ = 0;

private:
    std::shared_ptr<PageProcessorGpu> processor_;
    std::shared_ptr<FusedAggGpu> fused_;
};

FusedFilterProjectAggregationOperatorFactory::FusedFilterProjectAggregationOperatorFactory(Context *ctx, int32_t operator_id, std::vector<int32_t> input_types,
                                                                                           const tgpu_page_processor_spec *spec, HashAggregationConfig cfg)
    : ctx_(ctx), operator_id_(operator_id), cfg_(std::move(cfg))
{
    processor_ = PageProcessorGpu::shared(input_types, spec);
    const std::vector<int32_t> &pt = processor_->output_types();
    TG_CHECK_ARG(cfg_.group_by_types.size() == cfg_.group_by_channels.size(), "group-by types and channels differ in length");
    for (size_t i = 0; i < cfg_.group_by_channels.size(); i++) {
        const int32_t ch = cfg_.group_by_channels[i];
        TG_CHECK_ARG(ch >= 0 && ch < (int)pt.size() && pt[(size_t)ch] == cfg_.group_by_types[i], "group-by channel / type does not match the projections");
    }
    TG_CHECK_ARG(cfg_.hash_channel < (int)pt.size(), "hash channel out of range");
    TG_CHECK_ARG(cfg_.expected_groups > 0, "expectedGroups must be positive");
    for (const tgpu_agg_spec &a : cfg_.aggs)
        if (agg_is_varchar_extreme(a.function)) fail(TGPU_ERR_NOT_SUPPORTED, "min / max over VARCHAR is not supported by the fused filter / project aggregation");
    fused_ = FusedAggGpu::shared(input_types, spec, cfg_.aggs, cfg_.group_by_channels);
}

std::unique_ptr<Operator> FusedFilterProjectAggregationOperatorFactory::create_operator()
{
    check_open();
    return std::make_unique<FusedFilterProjectAggregationOperator>(ctx_, operator_id_, cfg_, processor_, fused_);
}

std::unique_ptr<OperatorFactory> FusedFilterProjectAggregationOperatorFactory::duplicate()
{
    return std::unique_ptr<OperatorFactory>(new FusedFilterProjectAggregationOperatorFactory(*this));
}

// =====================================================================================================================
// TopNOperator (M/operator/TopNOperator.java:135-225 over TopNProcessor.java:45-105): consumes pages until finish(), then emits
// the n first rows in sort order as one page
// =====================================================================================================================
class TopNOperator : public Operator {
public:
    TopNOperator(Context *ctx, int32_t id, const TopNConfig &cfg) : Operator(ctx, id), n_(cfg.n), top_(ctx, cfg.types, cfg.n, cfg.sort_channels, cfg.sort_orders) {}

    // :195-199 (n == 0: the operator is finished from the start and never wants input, :154-156)
    bool needs_input() override { return n_ > 0 && !finishing_; }

    void add_input(const tgpu_page *page) override
    {
        TG_CHECK_STATE(needs_input(), "Operator is already finishing");
        DevicePage in = ingest_page(ctx_, page);
        top_.add_page(in);
    }

    std::unique_ptr<OutputPage> get_output() override
    {
        if (n_ == 0 || !finishing_ || finished_) return nullptr;
        finished_ = true;
        DevicePage out = top_.result();
        if (out.n == 0) return nullptr;
        return wrap(std::move(out));
    }

    void finish() override { finishing_ = true; }
    bool is_finished() override { return n_ == 0 || finished_; }
    int64_t memory_bytes() override { return top_.estimated_size(); }

private:
    int64_t n_;
    TopNGpu top_;
    bool finishing_ = false, finished_ = false;
};

static void validate(Context *ctx, const TopNConfig &cfg)
{
    TopNGpu check(ctx, cfg.types, cfg.n, cfg.sort_channels, cfg.sort_orders);   // its constructor checks the arguments
    (void)check;
}

// =====================================================================================================================
// OrderByOperator (M/operator/OrderByOperator.java:160-300): PagesIndex.addPage per input page, one sort at finish()
// =====================================================================================================================
class OrderByOperator : public Operator {
public:
    OrderByOperator(Context *ctx, int32_t id, const OrderByConfig &cfg) : Operator(ctx, id), cfg_(cfg), index_(ctx, cfg.types) {}

    bool needs_input() override { return !finishing_; }

    void add_input(const tgpu_page *page) override
    {
        TG_CHECK_STATE(!finishing_, "Operator is already finishing");
        DevicePage in = ingest_page(ctx_, page);
        check_page_types(in, cfg_.types);
        index_.add_page(in);
    }

    std::unique_ptr<OutputPage> get_output() override
    {
        if (!finishing_ || finished_) return nullptr;
        finished_ = true;
        DevicePage all;
        all.n = index_.position_count();
        if (all.n == 0) return nullptr;
        for (size_t i = 0; i < cfg_.types.size(); i++) all.cols.push_back(index_.column((int)i));
        int64_t count = 0;
        BufferPtr pos = TopNGpu::sorted_positions(ctx_, all, cfg_.sort_channels, cfg_.sort_orders, all.n, count);
        DevicePage out;
        out.n = count;
        for (int32_t ch : cfg_.output_channels) out.cols.push_back(k::gather_column(ctx_, all.cols[(size_t)ch], pos->as<int32_t>(), count, false));
        return wrap(std::move(out));
    }

    void finish() override { finishing_ = true; }
    bool is_finished() override { return finished_ || (finishing_ && index_.position_count() == 0); }
    int64_t memory_bytes() override { return index_.estimated_size(); }

private:
    OrderByConfig cfg_;
    PagesIndexGpu index_;
    bool finishing_ = false, finished_ = false;
};

static void validate(Context *ctx, const OrderByConfig &cfg)
{
    TopNGpu check(ctx, cfg.types, 1, cfg.sort_channels, cfg.sort_orders);   // validates types / sort channels / sort orders
    (void)check;
    for (int32_t ch : cfg.output_channels) TG_CHECK_ARG(ch >= 0 && ch < (int)cfg.types.size(), "output channel out of range");
}

// =====================================================================================================================
// MergeOperator (M/operator/MergeOperator.java:44-256; the same routine behind LocalMergeSourceOperator.java:39-): a source operator
// over k sorted page streams, MergeSortedPages.mergeSortedPages (M/util/MergeSortedPages.java:41-142) as ROUNDS on the device.
// get_output pulls from every unfinished stream that holds fewer than half its read-ahead of rows, then runs at most one round (merge.h):
// the rows no later row of any stream can precede are merged and emitted, the others stay buffered.  A stream's buffered rows are ONE
// page: a pulled page is kept as it came (owners shared) while it is the only one, and rows left over from earlier pages are
// concatenated with the new ones into a buffer of the stream's own (PagesIndexGpu) when it pulls again.
// =====================================================================================================================
class MergeOperator : public Operator {
public:
    MergeOperator(Context *ctx, int32_t id, const MergeConfig &cfg)
        : Operator(ctx, id), cfg_(cfg), merge_(std::make_unique<MergeGpu>(ctx, cfg.types, cfg.output_channels, cfg.sort_channels, cfg.sort_orders))
    {
    }
    ~MergeOperator() override { close(); }

    bool is_source() const override { return true; }
    bool needs_input() override { return false; }                                                                    // :222-225
    void add_input(const tgpu_page *) override { fail(TGPU_ERR_NOT_SUPPORTED, "MergeOperator is a source operator"); }   // :228-231

    void add_page_source(const tgpu_page_source *src)                                                                // addSplit :155-177
    {
        TG_CHECK_ARG(src && src->get_next_page && src->is_finished, "page source callbacks are null");
        TG_CHECK_STATE(!no_more_splits_, "noMoreSplits has been called already");                                    // :159
        if (closed_) {   // a split that arrives after close: nothing will read it
            if (src->close) src->close(src->user);
            return;
        }
        streams_.emplace_back();
        streams_.back().source = *src;
    }
    void no_more_splits() { no_more_splits_ = true; }                                                                // :180-184

    // blockedOnSplits (:208-219) until noMoreSplits; afterwards the future of the first stream (in split order) that has no buffered row and
    // is waiting for its source -- the reference blocks on its sources one after the other (WorkProcessorUtils.mergeSorted :124-139)
    bool is_blocked() override
    {
        if (closed_) return false;
        if (!no_more_splits_) return true;
        for (Stream &s : streams_)
            if (waiting(s)) return !s.source.is_blocked || s.source.is_blocked(s.source.user) == 1;
        return false;
    }

    std::unique_ptr<OutputPage> get_output() override
    {
        if (closed_ || !no_more_splits_) return nullptr;
        const int64_t read_ahead = std::max<int64_t>(kMergeMinReadAheadRows, kMergeRoundRows / std::max<int64_t>(1, (int64_t)streams_.size()));
        for (Stream &s : streams_) pull(s, read_ahead);
        int64_t buffered = 0;
        for (Stream &s : streams_) {
            if (!s.finished && s.available() == 0) return nullptr;   // blocked on this stream: nothing is settled yet
            buffered += s.available();
        }
        if (buffered == 0) {   // every stream is finished and drained
            close();
            return nullptr;
        }
        // more buffered rows than one page may hold: every stream takes part with a window of its first rows, and a cut window counts
        // as an unfinished stream (its next row bounds the round); the rest comes out in later rounds
        const int64_t k = (int64_t)streams_.size(), share = std::max<int64_t>(1, kMergeMaxRoundRows / k);
        const bool cut = buffered > kMergeMaxRoundRows;
        std::vector<const DevicePage *> pages;
        std::vector<int64_t> head, window, settled;
        std::vector<bool> open;
        for (Stream &s : streams_) {
            const int64_t w = cut ? std::min(s.available(), share) : s.available();
            pages.push_back(s.has_buf ? &s.buf : nullptr);
            head.push_back(s.head);
            window.push_back(w);
            open.push_back(!s.finished || w < s.available());
        }
        DevicePage out = merge_->round(pages, head, window, open, settled);
        for (size_t i = 0; i < streams_.size(); i++) {
            Stream &s = streams_[i];
            s.head += settled[i];
            if (s.has_buf && s.available() == 0) s.drop();
        }
        bool done = true;
        for (Stream &s : streams_) done = done && s.finished && s.available() == 0;
        if (done) close();
        if (out.n == 0) return nullptr;
        return wrap(std::move(out));
    }

    void finish() override { close(); }                                                                              // :196-199
    bool is_finished() override
    {
        if (closed_) return true;
        if (!no_more_splits_) return false;
        for (Stream &s : streams_)
            if (!s.finished || s.available() > 0) return false;
        return true;   // (also: no split at all)
    }
    // the buffered input rows (whole buffers: rows already emitted leave with their buffer).  A round's page is handed out by the
    // get_output that built it, so no output page is ever pending here.
    int64_t memory_bytes() override
    {
        int64_t b = 0;
        for (Stream &s : streams_)
            if (s.has_buf) b += s.buf.size_in_bytes();
        return b;
    }
    void close() override                                                                                            // :240-255
    {
        for (Stream &s : streams_) {
            end(s);
            s.drop();
        }
        merge_.reset();
        closed_ = true;
    }

private:
    struct Stream {
        tgpu_page_source source{};
        bool source_open = true;   // its close callback has not been called
        bool finished = false;     // no further page will come
        bool last_zero = false;    // get_next_page returned 0 last
        bool has_buf = false;
        DevicePage buf;            // rows [head, buf.n) are buffered
        int64_t head = 0;
        int64_t available() const { return has_buf ? buf.n - head : 0; }
        void drop()
        {
            buf = DevicePage();
            has_buf = false;
            head = 0;
        }
    };
    static bool waiting(const Stream &s) { return !s.finished && s.available() == 0 && s.last_zero; }

    // the stream has ended (or the operator closes): its source is closed exactly once
    void end(Stream &s)
    {
        s.finished = true;
        if (s.source_open && s.source.close) s.source.close(s.source.user);
        s.source_open = false;
    }

    // Pulls once the stream holds fewer than HALF its read-ahead, then up to the read-ahead: rows left over from earlier pages are copied
    // when the stream pulls again (absorb), and a stream that can deliver takes in at least as many new rows as it carries over.
    void pull(Stream &s, int64_t read_ahead)
    {
        if (s.finished || s.available() >= std::max<int64_t>(1, read_ahead / 2)) return;
        std::vector<DevicePage> fresh;
        try {
            int64_t rows = s.available();
            while (rows < read_ahead) {
                if (s.source.is_finished(s.source.user) == 1) {
                    end(s);
                    break;
                }
                tgpu_page page{};
                const int32_t rc = s.source.get_next_page(s.source.user, &page);
                if (rc < 0) fail(rc, "the page source of a merged stream failed");
                if (rc == 0) {
                    if (s.source.is_finished(s.source.user) == 1) end(s);
                    else s.last_zero = true;
                    break;
                }
                s.last_zero = false;
                TG_CHECK_ARG(page.channel_count == (int32_t)cfg_.types.size(), "page channel count does not match the operator's types");
                for (int32_t ch = 0; ch < page.channel_count; ch++) {
                    TG_CHECK_ARG(page.blocks && page.blocks[ch].type == cfg_.types[(size_t)ch], "page channel type does not match the operator's types");
                    TG_CHECK_ARG(page.blocks[ch].encoding != TGPU_LAZY, "a merged stream's pages must be loaded");
                }
                if (page.position_count == 0) continue;
                TG_CHECK_STATE(rows + page.position_count <= 0xffffffffLL, "a merged stream buffers more rows than a row reference can address");
                DevicePage in = ingest_page(ctx_, &page);   // (host arrays are consumed when it returns)
                own_borrowed_columns(ctx_, in);             // device arrays are valid until the next call on the source only
                rows += in.n;
                fresh.push_back(std::move(in));
            }
        }
        catch (...) {
            // the pages this call took in before the failure are rows of the stream like any other: they stay buffered, so a caller that
            // goes on after the error loses nothing but the page that failed
            try {
                absorb(s, fresh);
            }
            catch (...) {
            }
            throw;
        }
        absorb(s, fresh);
    }

    // the stream's buffer becomes (rows not emitted yet, fresh pages...): one page kept as it came while it is the only one, else one
    // concatenation into a buffer of the stream's own
    void absorb(Stream &s, std::vector<DevicePage> &fresh)
    {
        if (fresh.empty()) return;
        if (s.available() == 0 && fresh.size() == 1) {
            s.buf = std::move(fresh[0]);
            s.head = 0;
            s.has_buf = true;
            fresh.clear();
            return;
        }
        PagesIndexGpu index(ctx_, cfg_.types);
        if (s.available() > 0) {
            DevicePage rest;
            rest.n = s.available();
            for (const DeviceColumn &c : s.buf.cols) rest.cols.push_back(k::region_of(ctx_, c, s.head, rest.n));
            index.add_page(rest);
        }
        for (const DevicePage &p : fresh) index.add_page(p);
        DevicePage all;
        all.n = index.position_count();
        for (size_t i = 0; i < cfg_.types.size(); i++) all.cols.push_back(index.column((int)i));
        s.buf = std::move(all);
        s.head = 0;
        s.has_buf = true;
        fresh.clear();
    }

    MergeConfig cfg_;
    std::unique_ptr<MergeGpu> merge_;
    std::vector<Stream> streams_;
    bool no_more_splits_ = false, closed_ = false;
};

static void validate(Context *ctx, const MergeConfig &cfg)
{
    MergeGpu check(ctx, cfg.types, cfg.output_channels, cfg.sort_channels, cfg.sort_orders);   // its constructor checks the arguments
    (void)check;
}

static MergeOperator *as_merge(Operator *op)
{
    auto *p = dynamic_cast<MergeOperator *>(op);
    TG_CHECK_ARG(p != nullptr, "not a MergeOperator");
    return p;
}
void merge_add_page_source(Operator *op, const tgpu_page_source *source) { as_merge(op)->add_page_source(source); }
void merge_no_more_splits(Operator *op) { as_merge(op)->no_more_splits(); }

// =====================================================================================================================
// DynamicFilterSourceOperator (M/operator/DynamicFilterSourceOperator.java:145-425).  Pages pass through unchanged (:375-381);
// per filter channel the operator keeps the set of distinct values (TypedSet -> a GroupByHash per channel here) while no
// channel exceeds max_distinct_values and the collected blocks stay within max_filter_size_in_bytes (:238-262); beyond that it
// falls back to min / max per orderable channel (:264-289, 291-338) as long as at most min_max_collection_limit rows were seen,
// and to "all" after that (:283-289).  finish() publishes the domains (:383-424): distinct non-null non-NaN values, or a
// [min, max] range, NONE for a channel that only saw nulls, ALL otherwise.
// Deviations, both on the safe side of an advisory filter (any superset of the build values is a valid dynamic filter):
// the size test uses the reference's BLOCK accounting of the collected values ((width + 1) or (length + 5) bytes per value)
// instead of TypedSet's JVM retained size.  min / max is kept for every orderable type of the path but DOUBLE, like the reference
// (:187-190): BIGINT / INTEGER / DATE / BOOLEAN by a reduction kernel, VARCHAR by selecting the first row in ascending and in
// descending order (topn.h: the type's comparison, bytes as unsigned) among the page's values and the running pair.
// =====================================================================================================================
namespace {
__global__ void __launch_bounds__(256) df_minmax_kernel(ColView col, int64_t n, long long *minmax /* [min, max, any non-null] */)
{
    long long lo = 0x7fffffffffffffffLL, hi = -0x7fffffffffffffffLL - 1;
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256) {
        if (col.nulls && col.nulls[r]) continue;
        const long long v = col.type == TGPU_BIGINT || col.type == TGPU_TIMESTAMP ? ((const long long *)col.values)[r]
                            : (col.type == TGPU_BOOLEAN ? (long long)(((const unsigned char *)col.values)[r] != 0) : (long long)((const int *)col.values)[r]);
        lo = v < lo ? v : lo;
        hi = v > hi ? v : hi;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const long long l2 = __shfl_down(lo, d, 64), h2 = __shfl_down(hi, d, 64);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
    }
    if ((threadIdx.x & 63) == 0 && lo <= hi) {
        atomicMin(&minmax[0], lo);
        atomicMax(&minmax[1], hi);
        minmax[2] = 1;
    }
}
// keep[i] = the distinct value i is neither null nor NaN (convertToDomain, :402-417)
__global__ void __launch_bounds__(256) df_keep_kernel(ColView col, int64_t n, int32_t *keep)
{
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256) {
        bool ok = !(col.nulls && col.nulls[r]);
        if (ok && col.type == TGPU_DOUBLE) {
            const double v = ((const double *)col.values)[r];
            ok = v == v;
        }
        keep[r] = ok ? 1 : 0;
    }
}
}  // namespace

class DynamicFilterSourceOperator : public Operator {
public:
    DynamicFilterSourceOperator(Context *ctx, int32_t id, const DynamicFilterSourceConfig &cfg)
        : Operator(ctx, id), types_(cfg.types), channels_(cfg.channels), max_distinct_(cfg.max_distinct_values), max_size_(cfg.max_filter_size_in_bytes),
          min_max_limit_(cfg.min_max_collection_limit)
    {
        for (int32_t ch : channels_) {
            const int32_t t = types_[(size_t)ch];
            sets_.push_back(std::make_unique<GroupByHashGpu>(ctx, std::vector<int32_t>{t}, false, 1024));
            const bool orderable = min_max_limit_ > 0 && t != TGPU_DOUBLE;   // :187-190 (orderable, DOUBLE / REAL left out because of NaN)
            if (orderable) min_max_channels_.push_back((int)sets_.size() - 1);
        }
        collecting_sets_ = true;
        collecting_min_max_ = !min_max_channels_.empty();
        if (collecting_min_max_) {
            minmax_ = ctx_->alloc(channels_.size() * 24);
            std::vector<long long> init;
            for (size_t k = 0; k < channels_.size(); k++) init.insert(init.end(), {0x7fffffffffffffffLL, -0x7fffffffffffffffLL - 1, 0});
            ctx_->upload(minmax_->ptr(), init.data(), init.size() * 8);
            ctx_->sync();
        }
    }

    bool needs_input() override { return !current_ && !finished_; }   // :208-211

    void add_input(const tgpu_page *page) override { collect(ingest_page(ctx_, page), true); }
    void add_input_owned(const DevicePage &page) override { collect(DevicePage(page), false); }

    std::unique_ptr<OutputPage> get_output() override { return std::move(current_); }   // :375-381

    void finish() override { finished_ = true; }   // the domains are read through dynamic_filter_result (:383-400)
    bool is_finished() override { return finished_ && !current_; }
    int64_t memory_bytes() override
    {
        int64_t s = current_ ? current_->page.size_in_bytes() : 0;
        for (auto &g : sets_) s += g ? g->estimated_size() : 0;
        return s;
    }

    void result(int32_t k, int32_t *kind, std::unique_ptr<OutputPage> *values, int64_t *min, int64_t *max)
    {
        TG_CHECK_STATE(finished_, "the dynamic filter is available after finish()");
        TG_CHECK_ARG(k >= 0 && k < (int)channels_.size(), "filter channel out of range");
        *kind = 0;
        *min = *max = 0;
        if (collecting_sets_) {   // :393-399 convertToDomain
            DevicePage keys = sets_[(size_t)k]->key_page(false);
            const int64_t n = keys.n;
            DevicePage out;
            out.n = 0;
            if (n > 0) {
                BufferPtr keep = ctx_->alloc((size_t)n * 4), rank = ctx_->alloc((size_t)n * 4), pos = ctx_->alloc((size_t)n * 4), total = ctx_->alloc(8);
                df_keep_kernel<<<(int)std::min<int64_t>(ceil_div(n, 256), 1024), 256, 0, ctx_->stream()>>>(view_of(keys.cols[0]), n, keep->as<int32_t>());
                k::exclusive_scan_i32(ctx_, keep->as<int32_t>(), rank->as<int32_t>(), n, total->as<int64_t>());
                k::compact_positions(ctx_, keep->as<int32_t>(), rank->as<int32_t>(), n, pos->as<int32_t>());
                check_launch("df_compact");
                out.n = ctx_->read_scalar(total->as<int64_t>());
                out.cols.push_back(k::gather_column(ctx_, keys.cols[0], pos->as<int32_t>(), out.n, false));
            }
            else out.cols.push_back(keys.cols[0]);
            *kind = 1;
            *values = wrap(std::move(out));
            return;
        }
        if (!collecting_min_max_) return;   // ALL (:386-390)
        bool is_mm = false;
        for (int c : min_max_channels_) is_mm = is_mm || c == k;
        if (!is_mm) return;                 // a channel without min / max collection is left out of the tuple domain = ALL
        if (types_[(size_t)channels_[(size_t)k]] == TGPU_VARCHAR) {
            auto it = varchar_min_max_.find(k);
            if (it == varchar_min_max_.end()) {
                *kind = 3;   // no value was ever seen
                return;
            }
            DevicePage pair;   // rows: min, max (both null when every value was null: ASC / DESC NULLS LAST put a null first only then)
            pair.n = 2;
            pair.cols.push_back(it->second);
            uint8_t null_flags[2] = {0, 0};
            if (it->second.nulls) ctx_->download(null_flags, it->second.nulls, 2);
            if (null_flags[0]) {
                *kind = 3;
                return;
            }
            *kind = 2;
            *values = wrap(std::move(pair));
            return;
        }
        long long mm[3];
        ctx_->download(mm, minmax_->as<long long>() + 3 * k, 24);
        if (!mm[2]) {
            *kind = 3;   // all values were null: Domain.none (:366-369)
            return;
        }
        *kind = 2;
        *min = mm[0];
        *max = mm[1];
    }

private:
    void collect(DevicePage in, bool borrowed)
    {
        TG_CHECK_STATE(needs_input(), "DynamicFilterSourceOperator: addInput() may not be called after finish() or with a pending page");
        check_page_types(in, types_);
        const int64_t n = in.n;
        if (collecting_sets_) {   // :236-262
            min_max_limit_left_sub(n);
            int64_t size = 0, most = 0;
            BufferPtr gids = ctx_->alloc((size_t)(n > 0 ? n : 1) * 4);
            for (size_t k = 0; k < channels_.size(); k++) {
                const DeviceColumn &c = in.cols[(size_t)channels_[k]];
                if (n > 0) sets_[k]->get_group_ids({&c}, nullptr, n, gids->as<int32_t>());
                const int64_t d = sets_[k]->group_count();
                most = std::max(most, d);
                DevicePage keys = sets_[k]->key_page(false);
                size += keys.cols[0].type == TGPU_VARCHAR ? keys.cols[0].pool_bytes + 5 * d : (int64_t)(type_width(keys.cols[0].type) + 1) * d;
            }
            if (most > max_distinct_ || size > max_size_) too_large();
        }
        else if (collecting_min_max_) {   // :218-233
            min_max_limit_left_sub(n);
            if (min_max_limit_left_ < 0) collecting_min_max_ = false;   // handleMinMaxCollectionLimitExceeded: ALL
            else
                for (int k : min_max_channels_) update_min_max(k, in.cols[(size_t)channels_[(size_t)k]]);
        }
        // the page itself goes on unchanged; a borrowed (device-resident) input is copied once so that it outlives the call
        if (borrowed) {
            bool needs_copy = false;
            for (auto &c : in.cols) needs_copy = needs_copy || (c.n > 0 && !c.values_buf);
            if (needs_copy) {
                PagesIndexGpu copy(ctx_, types_);
                copy.add_page(in);
                DevicePage owned;
                owned.n = in.n;
                for (size_t i = 0; i < types_.size(); i++) owned.cols.push_back(copy.column((int)i));
                in = std::move(owned);
            }
        }
        current_ = wrap(std::move(in));
    }

    void min_max_limit_left_sub(int64_t n)
    {
        if (!limit_started_) {
            min_max_limit_left_ = min_max_limit_;
            limit_started_ = true;
        }
        min_max_limit_left_ -= n;
    }

    void update_min_max(int k, const DeviceColumn &c)
    {
        if (c.n <= 0) return;
        if (c.type == TGPU_VARCHAR) {
            // candidates = the running (min, max) pair + this page's values; the new pair = the first row in ascending and the first in
            // descending order, nulls last (updateMinMaxValues :300-345 compares with the type's comparison operator)
            PagesIndexGpu cand(ctx_, std::vector<int32_t>{TGPU_VARCHAR});
            auto it = varchar_min_max_.find(k);
            if (it != varchar_min_max_.end()) {
                DevicePage prev;
                prev.n = 2;
                prev.cols.push_back(it->second);
                cand.add_page(prev);
            }
            DevicePage pg;
            pg.n = c.n;
            pg.cols.push_back(c);
            cand.add_page(pg);
            DevicePage all;
            all.n = cand.position_count();
            all.cols.push_back(cand.column(0));
            int64_t cnt = 0;
            BufferPtr lo = TopNGpu::sorted_positions(ctx_, all, {0}, {TGPU_SORT_ASC_NULLS_LAST}, 1, cnt);
            BufferPtr hi = TopNGpu::sorted_positions(ctx_, all, {0}, {TGPU_SORT_DESC_NULLS_LAST}, 1, cnt);
            BufferPtr both = ctx_->alloc(8);
            HIP_CHECK(hipMemcpyAsync(both->ptr(), lo->ptr(), 4, hipMemcpyDeviceToDevice, ctx_->stream()));
            HIP_CHECK(hipMemcpyAsync(both->as<int32_t>() + 1, hi->ptr(), 4, hipMemcpyDeviceToDevice, ctx_->stream()));
            varchar_min_max_[k] = k::gather_column(ctx_, all.cols[0], both->as<int32_t>(), 2, false);
            return;
        }
        df_minmax_kernel<<<(int)std::min<int64_t>(ceil_div(c.n, 256), (int64_t)ctx_->cu_count() * 2), 256, 0, ctx_->stream()>>>(view_of(c), c.n, minmax_->as<long long>() + 3 * k);
        check_launch("df_minmax");
    }

    void too_large()   // handleTooLargePredicate (:264-281)
    {
        if (min_max_channels_.empty() || min_max_limit_left_ < 0) collecting_min_max_ = false;   // ALL
        else
            for (int k : min_max_channels_) {   // min / max of what was collected so far = of every row seen so far
                DevicePage keys = sets_[(size_t)k]->key_page(false);
                update_min_max(k, keys.cols[0]);
            }
        collecting_sets_ = false;
        for (auto &g : sets_) g.reset();
    }

    std::vector<int32_t> types_, channels_;
    int32_t max_distinct_;
    int64_t max_size_;
    int32_t min_max_limit_;
    int64_t min_max_limit_left_ = 0;
    bool limit_started_ = false, collecting_sets_ = false, collecting_min_max_ = false, finished_ = false;
    std::vector<std::unique_ptr<GroupByHashGpu>> sets_;
    std::vector<int> min_max_channels_;
    BufferPtr minmax_;
    std::map<int, DeviceColumn> varchar_min_max_;   // filter channel -> 2 rows (min, max)
    std::unique_ptr<OutputPage> current_;
};

static void validate(Context *, const DynamicFilterSourceConfig &cfg)
{
    for (int32_t t : cfg.types) TG_CHECK_ARG(valid_type(t), "unknown type");
    std::set<int32_t> seen;
    for (int32_t ch : cfg.channels) {
        TG_CHECK_ARG(ch >= 0 && ch < (int)cfg.types.size(), "filter channel out of range");
        TG_CHECK_ARG(seen.insert(ch).second, "duplicate channel indices are not allowed");   // :105-106
    }
    TG_CHECK_ARG(cfg.max_distinct_values >= 0 && cfg.max_filter_size_in_bytes >= 0, "limits must not be negative");
}

std::unique_ptr<OperatorFactory> DynamicFilterSourceOperatorFactory::duplicate()
{
    // DynamicFilterSourceOperator.java:131-135: "duplicate() is not supported for DynamicFilterSourceOperatorFactory"
    fail(TGPU_ERR_NOT_SUPPORTED, "duplicate() is not supported for DynamicFilterSourceOperatorFactory");
}

void dynamic_filter_result(Operator *op, int32_t k, int32_t *kind, std::unique_ptr<OutputPage> *values, int64_t *min, int64_t *max)
{
    auto *p = dynamic_cast<DynamicFilterSourceOperator *>(op);
    TG_CHECK_ARG(p != nullptr, "not a DynamicFilterSourceOperator");
    p->result(k, kind, values, min, max);
}

// =====================================================================================================================
// SetBuilderOperator (M/operator/SetBuilderOperator.java:137-233): a sink.  The key channel of every page goes into the set (semijoin.h);
// finish() builds it and publishes it to the probes through the SetSupplier.  A precomputed hash channel is accepted and not read: the
// set hashes its keys itself (observable behaviour is the same: ChannelSet.contains compares keys).
// =====================================================================================================================
class SetBuilderOperator : public Operator {
public:
    SetBuilderOperator(Context *ctx, int32_t id, const std::vector<int32_t> &types, int32_t set_channel, std::shared_ptr<SetSupplier> supplier)
        : Operator(ctx, id), types_(types), set_channel_(set_channel), supplier_(std::move(supplier)),
          set_(std::make_shared<SemiSetGpu>(ctx, types[(size_t)set_channel]))
    {
    }

    bool needs_input() override { return !finished_; }   // :204-207
    void add_input(const tgpu_page *page) override { add(ingest_page(ctx_, page)); }
    void add_input_owned(const DevicePage &page) override { add(page); }
    std::unique_ptr<OutputPage> get_output() override { return nullptr; }   // :224-228

    void finish() override   // :180-196
    {
        if (finished_) return;
        set_->finish();
        supplier_->publish(set_);
        finished_ = true;
    }
    bool is_finished() override { return finished_; }
    // what the builder holds until it is closed: the collected keys, then the set (the probes share it through the supplier)
    int64_t memory_bytes() override { return closed_ || !set_ ? 0 : set_->estimated_size(); }
    void close() override
    {
        closed_ = true;
        set_.reset();
    }

private:
    void add(const DevicePage &in)   // :209-222
    {
        TG_CHECK_STATE(!finished_, "Operator is already finishing");
        check_page_types(in, types_);
        set_->add_keys(in.cols[(size_t)set_channel_]);
    }

    std::vector<int32_t> types_;
    int32_t set_channel_;
    std::shared_ptr<SetSupplier> supplier_;
    std::shared_ptr<SemiSetGpu> set_;
    bool finished_ = false, closed_ = false;
};

SetBuilderOperatorFactory::SetBuilderOperatorFactory(Context *ctx, int32_t operator_id, std::vector<int32_t> types, int32_t set_channel, int32_t hash_channel,
                                                     std::shared_ptr<SetSupplier> supplier)
    : ctx_(ctx), operator_id_(operator_id), types_(std::move(types)), set_channel_(set_channel), supplier_(std::move(supplier))
{
    TG_CHECK_ARG(!types_.empty(), "the set builder needs at least one channel");
    for (int32_t t : types_) TG_CHECK_ARG(valid_type(t), "unknown type");
    TG_CHECK_ARG(set_channel_ >= 0 && set_channel_ < (int)types_.size(), "set channel out of range");
    TG_CHECK_ARG(hash_channel >= -1 && hash_channel < (int)types_.size(), "hash channel out of range");
    TG_CHECK_ARG(supplier_->type() == types_[(size_t)set_channel_], "the supplier's type is not the set channel's type");
}

std::unique_ptr<Operator> SetBuilderOperatorFactory::create_operator()
{
    check_open();
    return std::make_unique<SetBuilderOperator>(ctx_, operator_id_, types_, set_channel_, supplier_);
}

// =====================================================================================================================
// HashSemiJoinOperator (M/operator/HashSemiJoinOperator.java:166-218): the input page's channels unchanged, then one BOOLEAN channel;
// one output page per input page.  Blocked, and taking no input, until the set is published -- as this library's LookupJoinOperator; a
// probe finished before that ends without output.  A DICTIONARY / RLE key block is probed once per dictionary entry and the results are
// gathered through its ids.
// =====================================================================================================================
class HashSemiJoinOperator : public PageOperator {
public:
    HashSemiJoinOperator(Context *ctx, int32_t id, const HashSemiJoinConfig &cfg)
        : PageOperator(ctx, id), supplier_(cfg.supplier), probe_types_(cfg.probe_types), channel_(cfg.probe_join_channel)
    {
    }

    bool is_blocked() override { return !finishing_ && !supplier_->set(); }
    bool needs_input() override { return !finishing_ && !pending_ && !is_blocked(); }

    void add_input(const tgpu_page *page) override
    {
        ready();
        TG_CHECK_ARG(page != nullptr, "page is null");
        TG_CHECK_ARG(page->channel_count == (int32_t)probe_types_.size(), "page channel count does not match the operator's types");
        const tgpu_block &kb = page->blocks[channel_];
        DeviceColumn verdict;
        bool have_verdict = false;
        if (kb.encoding != TGPU_FLAT && kb.dictionary != nullptr && kb.dictionary->encoding == TGPU_FLAT) {
            TG_CHECK_ARG(kb.type == probe_types_[(size_t)channel_], "page channel type does not match the operator's types");
            TG_CHECK_ARG(kb.position_count == page->position_count, "block position count differs from the page's");
            DeviceColumn dict;
            BufferPtr ids;
            ingest_dictionary(ctx_, &kb, dict, ids);
            verdict = k::gather_column(ctx_, supplier_->set()->probe(dict), ids->as<int32_t>(), page->position_count, false);
            have_verdict = true;
        }
        probe(ingest_page(ctx_, page), have_verdict ? &verdict : nullptr);
    }
    int64_t memory_bytes() override { return pending_ ? pending_->page.size_in_bytes() : 0; }

private:
    void ready() override
    {
        PageOperator::ready();
        TG_CHECK_STATE(supplier_->set() != nullptr, "ChannelSet has not been built yet");
    }
    void emit(DevicePage in) override { probe(std::move(in), nullptr); }

    void probe(DevicePage in, const DeviceColumn *verdict)
    {
        check_page_types(in, probe_types_);
        DeviceColumn out = verdict ? *verdict : supplier_->set()->probe(in.cols[(size_t)channel_]);
        // the page passes through: channels that borrow the caller's device memory get buffers of their own (the output outlives the call)
        own_borrowed_columns(ctx_, in);
        in.cols.push_back(std::move(out));
        pending_ = wrap(std::move(in));
    }

    std::shared_ptr<SetSupplier> supplier_;
    std::vector<int32_t> probe_types_;
    int32_t channel_;
};

static void validate(Context *, const HashSemiJoinConfig &cfg)
{
    TG_CHECK_ARG(!cfg.probe_types.empty(), "the semi join probe needs at least one channel");
    for (int32_t t : cfg.probe_types) TG_CHECK_ARG(valid_type(t), "unknown type");
    TG_CHECK_ARG(cfg.probe_join_channel >= 0 && cfg.probe_join_channel < (int)cfg.probe_types.size(), "probe join channel out of range");
    TG_CHECK_ARG(cfg.probe_hash_channel >= -1 && cfg.probe_hash_channel < (int)cfg.probe_types.size(), "probe hash channel out of range");
    TG_CHECK_ARG(cfg.probe_types[(size_t)cfg.probe_join_channel] == cfg.supplier->type(), "the probe key type is not the set's type");
}

// =====================================================================================================================
// NestedLoopBuildOperator (M/operator/NestedLoopBuildOperator.java:96-190): a sink.  Its pages stay in HBM as delivered
// (NestedLoopJoinPagesBuilder.java:45-110: empty pages dropped, pages without channels only counted and re-cut into pages of
// PageProcessor.MAX_BATCH_SIZE positions); finish() publishes them to the probes through the bridge.  Like the hash builder it then stays
// alive, blocked, until every probe operator has closed and the probe factories have seen noMoreOperators (:131-150).
// =====================================================================================================================
class NestedLoopBuildOperator : public Operator {
public:
    enum class State { CONSUMING_INPUT, PAGES_PUBLISHED, CLOSED };
    static constexpr int64_t kMaxBatchSize = 8192;   // PageProcessor.MAX_BATCH_SIZE

    NestedLoopBuildOperator(Context *ctx, int32_t id, std::shared_ptr<NestedLoopBridge> bridge)
        : Operator(ctx, id), bridge_(std::move(bridge)), pages_(std::make_shared<NestedLoopPages>())
    {
    }

    bool needs_input() override { return state_ == State::CONSUMING_INPUT; }
    void add_input(const tgpu_page *page) override
    {
        TG_CHECK_STATE(state_ == State::CONSUMING_INPUT, "Operator is already finishing");
        TG_CHECK_ARG(page != nullptr, "page is null");
        if (bridge_->build_types().empty()) {
            TG_CHECK_ARG(page->channel_count == 0 && page->position_count >= 0, "page channel count does not match the operator's types");
            count(page->position_count);
            return;
        }
        add(ingest_page(ctx_, page));
    }
    void add_input_owned(const DevicePage &page) override
    {
        TG_CHECK_STATE(state_ == State::CONSUMING_INPUT, "Operator is already finishing");
        add(DevicePage(page));
    }
    std::unique_ptr<OutputPage> get_output() override { return nullptr; }   // :176-180

    void finish() override   // :152-164
    {
        if (state_ != State::CONSUMING_INPUT) return;
        if (counter_ > 0) push_count(counter_);   // NestedLoopJoinPagesBuilder.build :100-105
        counter_ = 0;
        bridge_->publish(pages_);
        state_ = State::PAGES_PUBLISHED;
    }
    bool is_blocked() override { return state_ == State::PAGES_PUBLISHED && !bridge_->destroyed(); }
    bool is_finished() override
    {
        if (state_ == State::PAGES_PUBLISHED && bridge_->destroyed()) close();
        return state_ == State::CLOSED;
    }
    int64_t memory_bytes() override { return state_ == State::CLOSED || !pages_ ? 0 : pages_->bytes; }
    void close() override
    {
        state_ = State::CLOSED;
        pages_.reset();   // (the probes hold the published pages through the bridge)
    }

private:
    void add(DevicePage in)
    {
        check_page_types(in, bridge_->build_types());
        if (in.n == 0) return;
        if (in.cols.empty()) {
            count(in.n);
            return;
        }
        pages_->positions += in.n;
        pages_->bytes += in.size_in_bytes();
        pages_->pages.push_back(nl_keep(ctx_, std::move(in)));
    }
    void count(int64_t positions)   // updatePagePositionCounter :64-76
    {
        counter_ += positions;
        for (; counter_ >= kMaxBatchSize; counter_ -= kMaxBatchSize) push_count(kMaxBatchSize);
    }
    void push_count(int64_t positions)
    {
        NlPage pg;
        pg.page.n = positions;
        pages_->pages.push_back(std::move(pg));
        pages_->positions += positions;
    }

    std::shared_ptr<NestedLoopBridge> bridge_;
    std::shared_ptr<NestedLoopPages> pages_;
    int64_t counter_ = 0;
    State state_ = State::CONSUMING_INPUT;
};

NestedLoopBuildOperatorFactory::NestedLoopBuildOperatorFactory(Context *ctx, int32_t operator_id, std::shared_ptr<NestedLoopBridge> bridge)
    : ctx_(ctx), operator_id_(operator_id), bridge_(std::move(bridge))
{
    for (int32_t t : bridge_->build_types()) TG_CHECK_ARG(valid_type(t), "unknown type");
}

std::unique_ptr<Operator> NestedLoopBuildOperatorFactory::create_operator()
{
    check_open();
    return std::make_unique<NestedLoopBuildOperator>(ctx_, operator_id_, bridge_);
}

// =====================================================================================================================
// NestedLoopJoinOperator (M/operator/NestedLoopJoinOperator.java:154-274), alone or with a FilterAndProjectOperator fused behind it.
//
// The sequence: one probe page against each build page in turn; within a pair, one reference page per row of the small side, each the
// large side's L rows with the small row repeated (nested_loop.h) -- row r of the pair is (small row r / L, large row r % L).  The build
// page is the large side iff it has more rows; with no probe output channel a tie goes to the build page as well (PageRepeatingIterator,
// :265-267).  The operator hands that sequence out in pieces of its own size.
//
// Alone: every get_output materialises the next piece (nlj_product), at most max_rows rows and cut short where a VARCHAR channel's pool
// would reach 2^31 bytes; without output channels only counts come out, as few pages as the int32 position count allows.
//
// Fused: the spec's channels are (probe channels..., build channels...).  A filter the generator covers and that cannot raise is
// evaluated over the virtual product (NestedLoopFilterGpu: nlj_pair_count / nlj_pair_emit), whole small rows at a time or, where one
// small row's L pairs exceed max_rows, a range of large rows; the channels the projections read are gathered by the surviving pairs and
// a projection-only page processor runs over them.  Every other spec takes the unfused composition inside the operator: product pieces of
// the channels the spec reads, then the whole page processor.
//
// Errors.  The reference composition throws at the first reference page that fails, within it the filter before projection 0 before
// projection 1, then the first row.  Pieces are processed in sequence order, so the first piece that reports an error holds that page;
// which one it is, and what it throws, is found by running the piece's reference pages again one at a time, each WHOLE (a piece may hold
// part of one; the parts before it raised nothing): slow, exact, and only on the error path.
// =====================================================================================================================
struct NestedLoopPrograms {
    std::shared_ptr<NestedLoopFilterGpu> filter;          // the fused route when filter->supported()
    std::shared_ptr<PageProcessorGpu> all, proj;          // the whole spec / its projections alone, over the channels each reads
    std::vector<int> all_sources, proj_sources;           // compacted channel -> channel of the spec
};

namespace {
std::shared_ptr<PageProcessorGpu> compact_processor(const std::vector<int32_t> &types, const NestedLoopJoinConfig &cfg, bool with_filter, std::vector<int> &sources)
{
    tgpu_page_processor_spec spec{cfg.nodes.data(), (int32_t)cfg.nodes.size(), cfg.pool.data(), (int32_t)cfg.pool.size(), with_filter ? cfg.filter_root : -1,
                                  (int32_t)cfg.projection_roots.size(), cfg.projection_roots.data()};
    ExprProgram prog(types, &spec);
    std::set<int> read;
    if (spec.filter_root >= 0) prog.inputs_of(spec.filter_root, read);
    for (int32_t r : cfg.projection_roots) prog.inputs_of(r, read);
    // compacted as apply_join_filter does: the two sides together may have more than kFpMaxCols channels
    std::vector<int> remap(types.size(), -1);
    std::vector<int32_t> ctypes;
    for (int ch : read) {
        TG_CHECK_ARG(ch >= 0 && ch < (int)types.size(), "nested loop join: input channel out of range");
        remap[(size_t)ch] = (int)ctypes.size();
        ctypes.push_back(types[(size_t)ch]);
        sources.push_back(ch);
    }
    std::vector<tgpu_expr_node> nodes = cfg.nodes;
    for (auto &nd : nodes)
        if (nd.kind == TGPU_EX_INPUT && nd.op >= 0 && nd.op < (int)remap.size() && remap[(size_t)nd.op] >= 0) nd.op = remap[(size_t)nd.op];
    spec.nodes = nodes.data();
    return PageProcessorGpu::shared(ctypes, &spec);
}

bool is_expression_error(int32_t code)
{
    return code == TGPU_ERR_NUMERIC_VALUE_OUT_OF_RANGE || code == TGPU_ERR_DIVISION_BY_ZERO || code == TGPU_ERR_INVALID_CAST_ARGUMENT || code == TGPU_ERR_INVALID_ARGUMENT;
}
}  // namespace

class NestedLoopJoinOperator : public Operator {
public:
    NestedLoopJoinOperator(Context *ctx, int32_t id, const NestedLoopJoinConfig &cfg, std::shared_ptr<NestedLoopBridge> bridge, std::shared_ptr<NestedLoopPrograms> programs)
        : Operator(ctx, id), cfg_(cfg), bridge_(std::move(bridge)), programs_(std::move(programs))
    {
        const bool counts_only = !cfg_.fused && cfg_.probe_channels.empty() && cfg_.build_channels.empty();
        cap_ = cfg_.max_rows > 0 ? std::min(cfg_.max_rows, kNlMaxPositions) : (cfg_.fused ? kNlDefaultProductRows : counts_only ? kNlMaxPositions : kNlDefaultOutputRows);
        bridge_->probe_created();
    }
    ~NestedLoopJoinOperator() override { close(); }

    // blocked until the build side has published its pages (:171-175); an operator that is finishing without them has had no page
    bool is_blocked() override { return !closed_ && !finishing_ && !bridge_->pages(); }
    bool needs_input() override { return !closed_ && !finishing_ && !active_ && !is_blocked(); }   // :177-191
    void add_input(const tgpu_page *page) override
    {
        ready();
        start(ingest_page(ctx_, page));
    }
    void add_input_owned(const DevicePage &page) override
    {
        ready();
        start(DevicePage(page));
    }
    void finish() override { finishing_ = true; }
    bool is_finished() override   // :160-169
    {
        const bool done = closed_ || (finishing_ && !active_);
        if (done) close();
        return done;
    }
    int64_t memory_bytes() override { return active_ ? probe_.page.size_in_bytes() : 0; }
    void close() override
    {
        if (closed_) return;
        closed_ = true;
        end_page();
        build_.reset();
        bridge_->probe_closed();
    }

    std::unique_ptr<OutputPage> get_output() override   // :208-228
    {
        if (!active_) return nullptr;
        if (counts_left_ >= 0) {   // no output channel at all: position counts
            DevicePage out;
            out.n = std::min(cap_, counts_left_);
            counts_left_ -= out.n;
            if (counts_left_ == 0) end_page();
            return wrap(std::move(out));
        }
        const NlPage &bp = build_->pages[j_];
        Pair pr;
        pr.build = &bp;
        const int64_t p = probe_.page.n, b = bp.page.n;
        const bool probe_out = cfg_.fused ? !cfg_.probe_types.empty() : !cfg_.probe_channels.empty();
        const bool build_out = cfg_.fused ? !bridge_->build_types().empty() : !cfg_.build_channels.empty();
        pr.build_large = b > p || (b == p && !probe_out && build_out);
        pr.L = pr.build_large ? b : p;
        pr.S = pr.build_large ? p : b;
        const int64_t total = pr.S * pr.L;
        DevicePage out;
        int64_t rows = 0;
        bool have;
        if (!cfg_.fused) {
            rows = cut(pr, cfg_.probe_channels, cfg_.build_channels, r_, std::min(cap_, total - r_));
            out = product(pr, cfg_.probe_channels, cfg_.build_channels, r_, rows);
            have = true;
        }
        else have = filter_step(pr, total, out, rows);
        r_ += rows;
        if (r_ == total) {
            r_ = 0;
            if (++j_ == build_->pages.size()) end_page();
        }
        return have ? wrap(std::move(out)) : nullptr;
    }

private:
    struct Pair {
        const NlPage *build;
        bool build_large;
        int64_t L, S;
    };

    void ready()
    {
        TG_CHECK_STATE(!finishing_ && !closed_, "Operator is finishing");                                   // :197
        TG_CHECK_STATE(bridge_->pages() != nullptr, "Page source has not been built yet");                 // :198
        TG_CHECK_STATE(!active_, "Current page has not been completely processed yet");                    // :199
    }
    void start(DevicePage in)
    {
        check_page_types(in, cfg_.probe_types);
        build_ = bridge_->pages();
        if (in.n == 0 || build_->pages.empty()) return;   // :202-205; an empty build side gives nothing at all
        if (!cfg_.fused && cfg_.probe_channels.empty() && cfg_.build_channels.empty()) counts_left_ = in.n * build_->positions;
        probe_ = nl_keep(ctx_, std::move(in));
        active_ = true;
        j_ = 0;
        r_ = 0;
    }
    void end_page()
    {
        active_ = false;
        counts_left_ = -1;
        probe_ = NlPage();
    }

    // rows [r, r + n) of the pair: the probe channels, then the build channels
    DevicePage product(const Pair &pr, const std::vector<int32_t> &probe_channels, const std::vector<int32_t> &build_channels, int64_t r, int64_t n)
    {
        ProfileScope ps(ctx_, "nlj_product");
        DevicePage out;
        out.n = n;
        for (int32_t ch : probe_channels) out.cols.push_back(nl_product_column(ctx_, probe_, ch, !pr.build_large, pr.L, r, n));
        for (int32_t ch : build_channels) out.cols.push_back(nl_product_column(ctx_, *pr.build, ch, pr.build_large, pr.L, r, n));
        return out;
    }
    int64_t cut(const Pair &pr, const std::vector<int32_t> &probe_channels, const std::vector<int32_t> &build_channels, int64_t r, int64_t want)
    {
        return std::min(nl_cut_rows(probe_, probe_channels, !pr.build_large, pr.L, r, want), nl_cut_rows(*pr.build, build_channels, pr.build_large, pr.L, r, want));
    }

    // ---- fused ----
    void split_sources(const std::vector<int> &sources, std::vector<int32_t> &probe_channels, std::vector<int32_t> &build_channels) const
    {
        const int np = (int)cfg_.probe_types.size();
        for (int src : sources) (src < np ? probe_channels : build_channels).push_back(src < np ? src : src - np);
    }
    // the unfused composition over rows [r, r + n): product of the channels the spec reads, then the page processor
    bool process_rows(const Pair &pr, int64_t r, int64_t n, DevicePage &out)
    {
        std::vector<int32_t> pc, bc;
        split_sources(programs_->all_sources, pc, bc);   // (sources ascend: the probe's channels come first, as in the compacted page)
        DevicePage in = product(pr, pc, bc, r, n);
        return programs_->all->process(ctx_, in, out);
    }
    // the fused route over small rows [s, s + Sn) x large rows [l, l + Ln)
    bool process_pairs(const Pair &pr, int64_t s, int64_t Sn, int64_t l, int64_t Ln, DevicePage &out)
    {
        BufferPtr probe_idx, build_idx;
        const int64_t n = programs_->filter->pairs(ctx_, probe_.page, pr.build->page, pr.build_large, s, Sn, l, Ln, probe_idx, build_idx);
        if (n == 0) return false;
        DevicePage survivors;
        survivors.n = n;
        const int np = (int)cfg_.probe_types.size();
        {
            ProfileScope ps(ctx_, "nlj_gather");
            for (int src : programs_->proj_sources)
                survivors.cols.push_back(src < np ? k::gather_column(ctx_, probe_.page.cols[(size_t)src], probe_idx->as<int32_t>(), n, false)
                                                  : k::gather_column(ctx_, pr.build->page.cols[(size_t)(src - np)], build_idx->as<int32_t>(), n, false));
        }
        return programs_->proj->process(ctx_, survivors, out);
    }
    bool filter_step(const Pair &pr, int64_t total, DevicePage &out, int64_t &rows)
    {
        const bool fused_route = programs_->filter->supported();
        const int64_t s = r_ / pr.L, l = r_ - s * pr.L;
        int64_t Sn = 1, Ln = 0;
        if (fused_route) {
            if (l == 0 && pr.L <= cap_) {
                Sn = std::min(pr.S - s, cap_ / pr.L);
                Ln = pr.L;
            }
            else Ln = std::min(pr.L - l, cap_);
            rows = Sn * Ln;
        }
        else {
            std::vector<int32_t> pc, bc;
            split_sources(programs_->all_sources, pc, bc);
            rows = cut(pr, pc, bc, r_, std::min(cap_, total - r_));
        }
        try {
            return fused_route ? process_pairs(pr, s, Sn, l, Ln, out) : process_rows(pr, r_, rows, out);
        }
        catch (const Error &e) {
            if (!is_expression_error(e.code)) throw;
            // which reference page fails first, and with what: each page of the piece again, whole, in order
            for (int64_t page = s; page <= (r_ + rows - 1) / pr.L; page++) {
                DevicePage ignored;
                if (fused_route) process_pairs(pr, page, 1, 0, pr.L, ignored);
                else process_rows(pr, page * pr.L, pr.L, ignored);
            }
            throw;
        }
    }

    NestedLoopJoinConfig cfg_;
    std::shared_ptr<NestedLoopBridge> bridge_;
    std::shared_ptr<NestedLoopPrograms> programs_;
    std::shared_ptr<const NestedLoopPages> build_;
    NlPage probe_;
    size_t j_ = 0;               // the build page of the current pair
    int64_t r_ = 0;              // the next row of the pair's sequence
    int64_t counts_left_ = -1;   // >= 0: no output channel, the positions still to hand out for the probe page
    int64_t cap_ = 0;
    bool active_ = false, finishing_ = false, closed_ = false;
};

NestedLoopJoinOperatorFactory::NestedLoopJoinOperatorFactory(Context *ctx, int32_t operator_id, NestedLoopJoinConfig cfg, std::shared_ptr<NestedLoopBridge> bridge)
    : ctx_(ctx), operator_id_(operator_id), cfg_(std::move(cfg)), bridge_(std::move(bridge))
{
    for (int32_t t : cfg_.probe_types) TG_CHECK_ARG(valid_type(t), "unknown type");
    for (int32_t ch : cfg_.probe_channels) TG_CHECK_ARG(ch >= 0 && ch < (int)cfg_.probe_types.size(), "probe channel out of range");
    for (int32_t ch : cfg_.build_channels) TG_CHECK_ARG(ch >= 0 && ch < (int)bridge_->build_types().size(), "build channel out of range");
    TG_CHECK_ARG(cfg_.max_rows >= 0, "the row limit must be at least zero");
    if (cfg_.fused) {
        std::vector<int32_t> types = cfg_.probe_types;
        types.insert(types.end(), bridge_->build_types().begin(), bridge_->build_types().end());
        programs_ = std::make_shared<NestedLoopPrograms>();
        programs_->all = compact_processor(types, cfg_, true, programs_->all_sources);   // (checks the spec, whichever route it takes)
        tgpu_page_processor_spec spec{cfg_.nodes.data(), (int32_t)cfg_.nodes.size(), cfg_.pool.data(), (int32_t)cfg_.pool.size(), cfg_.filter_root,
                                      (int32_t)cfg_.projection_roots.size(), cfg_.projection_roots.data()};
        programs_->filter = NestedLoopFilterGpu::shared(cfg_.probe_types, bridge_->build_types(), &spec);
        if (programs_->filter->supported()) programs_->proj = compact_processor(types, cfg_, false, programs_->proj_sources);
    }
    bridge_->probe_factory_created();
}

std::unique_ptr<Operator> NestedLoopJoinOperatorFactory::create_operator()
{
    check_open();
    return std::make_unique<NestedLoopJoinOperator>(ctx_, operator_id_, cfg_, bridge_, programs_);
}

std::unique_ptr<OperatorFactory> NestedLoopJoinOperatorFactory::duplicate() { return std::make_unique<NestedLoopJoinOperatorFactory>(ctx_, operator_id_, cfg_, bridge_); }

void NestedLoopJoinOperatorFactory::no_more_operators()
{
    if (closed_) return;
    closed_ = true;
    bridge_->no_more_probes();
}

// =====================================================================================================================
// MarkDistinctOperator (M/operator/MarkDistinctOperator.java:94-203): the input page's channels unchanged, then one BOOLEAN channel
// without nulls that is true on the first row of every key the operator has not seen before (MarkDistinctHash.java:52-69); one output
// page per input page.  A null key is a group like any other.  DistinctLimitOperator (M/operator/DistinctLimitOperator.java:101-263):
// the distinct channels (+ the hash channel) of exactly those rows, cut at the remaining limit.  Both: one GroupByHashGpu per operator,
// then the marking kernels of distinct.hip.
// =====================================================================================================================
namespace {
void check_distinct_config(const std::vector<int32_t> &types, const std::vector<int32_t> &channels, int32_t hash_channel, const char *what)
{
    TG_CHECK_ARG(!types.empty(), std::string(what) + " needs at least one source channel");
    for (int32_t t : types) TG_CHECK_ARG(valid_type(t), "unknown type");
    TG_CHECK_ARG(!channels.empty(), std::string(what) + " needs at least one distinct channel");
    TG_CHECK_ARG((int)channels.size() <= kMaxKeyChannels, "at most 8 key channels are supported");
    for (int32_t ch : channels) TG_CHECK_ARG(ch >= 0 && ch < (int)types.size(), "distinct channel out of range");
    TG_CHECK_ARG(hash_channel >= -1 && hash_channel < (int)types.size(), "hash channel out of range");
    TG_CHECK_ARG(hash_channel < 0 || types[(size_t)hash_channel] == TGPU_BIGINT, "hash channel must be BIGINT");
}
}  // namespace

class MarkDistinctOperator : public PageOperator {   // needsInput :137-141, isFinished :131-135
public:
    MarkDistinctOperator(Context *ctx, int32_t id, const MarkDistinctConfig &cfg)
        : PageOperator(ctx, id), cfg_(cfg), marker_(ctx, types_of_channels(cfg.types, cfg.mark_channels), cfg.hash_channel >= 0, 10000)   // MarkDistinctHash.java:39
    {
    }
    int64_t memory_bytes() override { return marker_.estimated_size(); }

private:
    void emit(DevicePage in) override   // :143-174
    {
        check_page_types(in, cfg_.types);
        const auto [keys, hashes] = key_inputs(in, cfg_.mark_channels, cfg_.hash_channel);
        DeviceColumn mark = marker_.mark(keys, hashes, in.n);
        // the page passes through: channels that borrow the caller's device memory get buffers of their own (the output outlives the call)
        own_borrowed_columns(ctx_, in);
        in.cols.push_back(std::move(mark));
        pending_ = wrap(std::move(in));
    }

    MarkDistinctConfig cfg_;
    DistinctMarkerGpu marker_;
};

static void validate(Context *, const MarkDistinctConfig &cfg) { check_distinct_config(cfg.types, cfg.mark_channels, cfg.hash_channel, "mark distinct"); }

class DistinctLimitOperator : public PageOperator {
public:
    DistinctLimitOperator(Context *ctx, int32_t id, const DistinctLimitConfig &cfg)
        : PageOperator(ctx, id), cfg_(cfg), remaining_(cfg.limit),
          marker_(ctx, types_of_channels(cfg.types, cfg.distinct_channels), cfg.hash_channel >= 0,
                  (int32_t)std::max<int64_t>(1, std::min<int64_t>(cfg.limit, 10000)))   // :130-138 (a limit of 0 never sees a page)
    {
    }

    bool needs_input() override { return !finishing_ && remaining_ > 0 && !pending_; }       // :160-164
    bool is_finished() override { return !pending_ && (finishing_ || remaining_ == 0); }     // :154-158
    int64_t memory_bytes() override { return marker_.estimated_size(); }

private:
    void ready() override { TG_CHECK_STATE(needs_input(), "Operator does not need input"); }

    void emit(DevicePage in) override   // :166-223
    {
        check_page_types(in, cfg_.types);
        const auto [keys, hashes] = key_inputs(in, cfg_.distinct_channels, cfg_.hash_channel);
        const int32_t *positions = nullptr;
        const int64_t kept = marker_.first_rows(keys, hashes, in.n, remaining_, &positions);
        if (kept == 0) return;   // no output page for a page without a new key (:212-223)
        DevicePage out;
        out.n = kept;
        for (int32_t ch : cfg_.distinct_channels) out.cols.push_back(k::gather_column(ctx_, in.cols[(size_t)ch], positions, kept, false));
        if (cfg_.hash_channel >= 0) out.cols.push_back(k::gather_column(ctx_, in.cols[(size_t)cfg_.hash_channel], positions, kept, false));   // :125-128
        remaining_ -= kept;
        pending_ = wrap(std::move(out));
    }

    DistinctLimitConfig cfg_;
    int64_t remaining_;
    DistinctMarkerGpu marker_;
};

static void validate(Context *, const DistinctLimitConfig &cfg)
{
    check_distinct_config(cfg.types, cfg.distinct_channels, cfg.hash_channel, "distinct limit");
    TG_CHECK_ARG(cfg.limit >= 0, "limit must be at least zero");   // :70
}

// =====================================================================================================================
// RowNumberOperator (M/operator/RowNumberOperator.java:121-364): row_number() OVER (PARTITION BY k), with or without `<= n`.  Output =
// the output channels, then the BIGINT row number (len(outputChannels) + 1 channels in both modes; the reference's no-limit path sizes
// its block array by the INPUT page's channel count, :291, which leaves holes when the output channels are a strict subset -- not
// reproduced).  One page at a time: needs_input is false while a page's result is pending.  Partitioned: one GroupByHashGpu, then the
// ranking kernels of rownumber.hip.  Not partitioned: the count is a host int64 and the only kernel is the iota of the new column.
// =====================================================================================================================
class RowNumberOperator : public PageOperator {
public:
    RowNumberOperator(Context *ctx, int32_t id, const RowNumberConfig &cfg)
        : PageOperator(ctx, id), cfg_(cfg), max_rows_(cfg.max_rows_per_partition),
          numberer_(ctx, types_of_channels(cfg.types, cfg.partition_channels), cfg.hash_channel >= 0, cfg.expected_positions, cfg.max_rows_per_partition)
    {
        // TGPU_ROW_NUMBER_PATH=sort, read here: every page down the sort path instead of the choice by group count (the baseline of
        // tools/exp_row_number.py; the tests reach the sort path with few groups through it)
        const char *e = getenv("TGPU_ROW_NUMBER_PATH");
        numberer_.force_sort(e != nullptr && !strcmp(e, "sort"));
    }

    bool needs_input() override { return !single_partition_done() && PageOperator::needs_input(); }   // :201-209
    // :188-199; a partitioned operator never finishes early
    bool is_finished() override { return !pending_ && (finishing_ || single_partition_done()); }
    int64_t memory_bytes() override { return numberer_.estimated_size(); }   // :266

private:
    bool single_partition_done() const { return !numberer_.partitioned() && max_rows_ >= 0 && count_ == max_rows_; }
    void ready() override
    {
        PageOperator::ready();
        TG_CHECK_STATE(!single_partition_done(), "Operator does not need input");
    }

    void emit(DevicePage in) override   // :225-247
    {
        check_page_types(in, cfg_.types);
        DevicePage out;
        if (!numberer_.partitioned()) {
            const int64_t take = max_rows_ >= 0 ? std::min(in.n, max_rows_ - count_) : in.n;
            if (max_rows_ >= 0 && take == 0) return;   // an empty PageBuilder is no page (:335-337)
            for (int32_t ch : cfg_.output_channels) out.cols.push_back(in.cols[(size_t)ch]);
            own_borrowed_columns(ctx_, out);   // the channels pass through: the output outlives the call
            if (take < in.n)
                for (DeviceColumn &c : out.cols) c = k::region_of(ctx_, c, 0, take);
            out.n = take;
            out.cols.push_back(numberer_.iota(count_, take));
            count_ += take;
            pending_ = wrap(std::move(out));
            return;
        }
        const auto [keys, hashes] = key_inputs(in, cfg_.partition_channels, cfg_.hash_channel);
        if (max_rows_ < 0) {   // getRowsWithRowNumber (:289-299)
            DeviceColumn rn = numberer_.number(keys, hashes, in.n);
            for (int32_t ch : cfg_.output_channels) out.cols.push_back(in.cols[(size_t)ch]);
            own_borrowed_columns(ctx_, out);
            out.n = in.n;
            out.cols.push_back(std::move(rn));
            pending_ = wrap(std::move(out));
            return;
        }
        const int32_t *positions = nullptr;   // getSelectedRows (:313-342)
        DeviceColumn rn;
        const int64_t kept = numberer_.select(keys, hashes, in.n, &positions, &rn);
        if (kept == 0) return;
        out.n = kept;
        for (int32_t ch : cfg_.output_channels) out.cols.push_back(k::gather_column(ctx_, in.cols[(size_t)ch], positions, kept, false));
        out.cols.push_back(std::move(rn));
        pending_ = wrap(std::move(out));
    }

    RowNumberConfig cfg_;
    int64_t max_rows_;
    RowNumbererGpu numberer_;
    int64_t count_ = 0;   // partitionRowCount.get(0) of the single partition
};

static void validate(Context *, const RowNumberConfig &cfg)
{
    const int nt = (int)cfg.types.size();
    TG_CHECK_ARG(!cfg.types.empty(), "row number needs at least one source channel");
    for (int32_t t : cfg.types) TG_CHECK_ARG(valid_type(t), "unknown type");
    for (int32_t ch : cfg.output_channels) TG_CHECK_ARG(ch >= 0 && ch < nt, "output channel out of range");
    TG_CHECK_ARG((int)cfg.partition_channels.size() <= kMaxKeyChannels, "at most 8 key channels are supported");
    for (int32_t ch : cfg.partition_channels) TG_CHECK_ARG(ch >= 0 && ch < nt, "partition channel out of range");
    TG_CHECK_ARG(cfg.hash_channel >= -1 && cfg.hash_channel < nt, "hash channel out of range");
    TG_CHECK_ARG(cfg.hash_channel < 0 || !cfg.partition_channels.empty(), "a hash channel needs partition channels");
    TG_CHECK_ARG(cfg.hash_channel < 0 || cfg.types[(size_t)cfg.hash_channel] == TGPU_BIGINT, "hash channel must be BIGINT");
    TG_CHECK_ARG(cfg.max_rows_per_partition >= -1 && cfg.max_rows_per_partition <= 0x7fffffffLL, "max rows per partition must be -1 (none) or a non-negative int");
    TG_CHECK_ARG(cfg.expected_positions > 0, "expected positions must be positive");
}

// =====================================================================================================================
// TopNRankingOperator (M/operator/TopNRankingOperator.java:170-310): row_number() / rank() OVER (PARTITION BY k ORDER BY x) <= n.  Consumes
// pages until finish() (needsInput :261-266), then hands out the kept rows as ONE page (as TopNOperator and OrderByOperator do here):
// the output channels, then -- unless partial -- the BIGINT ranking (generateRanking, :99).  The work is GroupedTopNGpu's
// (topn_ranking.hip); rows that compare equal rank in arrival order.
// =====================================================================================================================
class TopNRankingOperator : public Operator {
public:
    TopNRankingOperator(Context *ctx, int32_t id, const TopNRankingConfig &cfg)
        : Operator(ctx, id), cfg_(cfg),
          top_(ctx, cfg.types, cfg.partition_channels, cfg.sort_channels, cfg.sort_orders, cfg.ranking_type, cfg.max_rank_per_partition, cfg.hash_channel,
               cfg.expected_positions)
    {
        // Switches, read here (as TGPU_ROW_NUMBER_PATH is): TGPU_TOP_N_RANKING_PREFILTER=off keeps every row of a page for the selection,
        // TGPU_TOP_N_RANKING_COMPACT_ROWS=<k> replaces the floor below which the store is not compacted.  The baselines of
        // tools/exp_top_n_ranking.py; the tests reach every path with small inputs through them.
        const char *e = getenv("TGPU_TOP_N_RANKING_PREFILTER");
        top_.set_prefilter(!(e != nullptr && !strcmp(e, "off")));
        e = getenv("TGPU_TOP_N_RANKING_COMPACT_ROWS");
        if (e != nullptr && *e) top_.set_compact_floor(std::max<int64_t>(1, strtoll(e, nullptr, 10)));
        e = getenv("TGPU_TOP_N_RANKING_SLICE_ROWS");   // a third one, for the tests alone: the slice length of GroupedTopNGpu::kSliceRows
        if (e != nullptr && *e) top_.set_slice_rows(std::max<int64_t>(1, strtoll(e, nullptr, 10)));
    }

    bool needs_input() override { return !finishing_; }   // :261-266

    void add_input(const tgpu_page *page) override
    {
        TG_CHECK_STATE(!finishing_, "Operator is already finishing");
        top_.add_page(ingest_page(ctx_, page));
    }

    std::unique_ptr<OutputPage> get_output() override
    {
        if (!finishing_ || finished_) return nullptr;
        finished_ = true;
        DeviceColumn ranking;
        DevicePage all = top_.result(&ranking);
        if (all.n == 0) return nullptr;
        DevicePage out;
        out.n = all.n;
        for (int32_t ch : cfg_.output_channels) out.cols.push_back(all.cols[(size_t)ch]);
        if (!cfg_.partial) out.cols.push_back(std::move(ranking));
        return wrap(std::move(out));
    }

    void finish() override { finishing_ = true; }
    bool is_finished() override { return finished_ || (finishing_ && top_.position_count() == 0); }
    int64_t memory_bytes() override { return top_.estimated_size(); }

private:
    TopNRankingConfig cfg_;
    GroupedTopNGpu top_;
    bool finishing_ = false, finished_ = false;
};

static void validate(Context *, const TopNRankingConfig &cfg)
{
    const int nt = (int)cfg.types.size();
    TG_CHECK_ARG(cfg.ranking_type != TGPU_RANKING_DENSE_RANK, "dense_rank is not supported");   // UnsupportedOperationException, TopNRankingOperator.java:235-236
    TG_CHECK_ARG(cfg.ranking_type == TGPU_RANKING_ROW_NUMBER || cfg.ranking_type == TGPU_RANKING_RANK, "unknown ranking type");
    TG_CHECK_ARG(!cfg.types.empty(), "top n ranking needs at least one source channel");
    for (int32_t t : cfg.types) TG_CHECK_ARG(valid_type(t), "unknown type");
    for (int32_t ch : cfg.output_channels) TG_CHECK_ARG(ch >= 0 && ch < nt, "output channel out of range");
    TG_CHECK_ARG((int)cfg.partition_channels.size() <= kMaxKeyChannels, "at most 8 partition channels are supported");
    for (int32_t ch : cfg.partition_channels) TG_CHECK_ARG(ch >= 0 && ch < nt, "partition channel out of range");
    TG_CHECK_ARG(!cfg.sort_channels.empty() && cfg.sort_channels.size() == cfg.sort_orders.size(), "sort channels and sort orders: at least one, equally many");
    TG_CHECK_ARG((int)cfg.sort_channels.size() <= kMaxKeyChannels, "at most 8 sort channels are supported");
    for (int32_t ch : cfg.sort_channels) TG_CHECK_ARG(ch >= 0 && ch < nt, "sort channel out of range");
    for (int32_t o : cfg.sort_orders) TG_CHECK_ARG(o >= TGPU_SORT_ASC_NULLS_FIRST && o <= TGPU_SORT_DESC_NULLS_LAST, "unknown sort order");
    TG_CHECK_ARG(cfg.max_rank_per_partition > 0 && cfg.max_rank_per_partition <= 0x7fffffffLL, "max rank per partition must be a positive int");   // :96, :199
    TG_CHECK_ARG(cfg.expected_positions > 0, "expected positions must be positive");
    TG_CHECK_ARG(cfg.hash_channel >= -1 && cfg.hash_channel < nt, "hash channel out of range");
    TG_CHECK_ARG(cfg.hash_channel < 0 || !cfg.partition_channels.empty(), "a hash channel needs partition channels");
    TG_CHECK_ARG(cfg.hash_channel < 0 || cfg.types[(size_t)cfg.hash_channel] == TGPU_BIGINT, "hash channel must be BIGINT");
}

// =====================================================================================================================
// WindowOperator (M/operator/WindowOperator.java:205-310): f(..) OVER (PARTITION BY k ORDER BY x <frame>).  Consumes pages into a PagesIndex
// until finish(), then hands out ONE page (as OrderByOperator does here): the output channels in sorted order, then one channel per window
// function.  The work is WindowGpu's (window.hip): the sort of OrderByOperator, then heads, one fused segmented scan and one launch per
// function.
// =====================================================================================================================
class WindowOperator : public Operator {
public:
    WindowOperator(Context *ctx, int32_t id, const WindowConfig &cfg)
        : Operator(ctx, id), cfg_(cfg), index_(ctx, cfg.types), window_(ctx, cfg.types, cfg.functions, cfg.partition_channels, cfg.sort_channels, cfg.sort_orders)
    {
        // TGPU_WINDOW_TILE_ROWS=<rows>, a multiple of 256, read here (as TGPU_TOP_N_RANKING_SLICE_ROWS is): the rows one workgroup of the scan
        // owns, so that the tests reach the multi-tile paths with small inputs
        const char *e = getenv("TGPU_WINDOW_TILE_ROWS");
        if (e != nullptr && *e) {
            const int64_t rows = strtoll(e, nullptr, 10);
            TG_CHECK_ARG(rows > 0 && rows % WindowGpu::kBlock == 0, "TGPU_WINDOW_TILE_ROWS must be a positive multiple of 256");
            window_.set_tile_rows(rows);
        }
    }

    bool needs_input() override { return !finishing_; }

    void add_input(const tgpu_page *page) override
    {
        TG_CHECK_STATE(!finishing_, "Operator is already finishing");
        DevicePage in = ingest_page(ctx_, page);
        check_page_types(in, cfg_.types);
        index_.add_page(in);
    }

    std::unique_ptr<OutputPage> get_output() override
    {
        if (!finishing_ || finished_) return nullptr;
        finished_ = true;
        DevicePage all;
        all.n = index_.position_count();
        if (all.n == 0) return nullptr;
        for (size_t i = 0; i < cfg_.types.size(); i++) all.cols.push_back(index_.column((int)i));
        BufferPtr pos;
        std::vector<DeviceColumn> functions = window_.evaluate(all, &pos);
        DevicePage out;
        out.n = all.n;
        for (int32_t ch : cfg_.output_channels)
            out.cols.push_back(pos ? k::gather_column(ctx_, all.cols[(size_t)ch], pos->as<int32_t>(), all.n, false) : all.cols[(size_t)ch]);
        for (DeviceColumn &c : functions) out.cols.push_back(std::move(c));
        return wrap(std::move(out));
    }

    void finish() override { finishing_ = true; }
    bool is_finished() override { return finished_ || (finishing_ && index_.position_count() == 0); }
    int64_t memory_bytes() override { return index_.estimated_size() + window_.scratch_bytes(); }   // index + what get_output took: positions + scan arrays

private:
    WindowConfig cfg_;
    PagesIndexGpu index_;
    WindowGpu window_;
    bool finishing_ = false, finished_ = false;
};

static void validate(Context *, const WindowConfig &cfg)
{
    WindowGpu::validate(cfg.types, cfg.functions, cfg.partition_channels, cfg.sort_channels, cfg.sort_orders);
    for (int32_t ch : cfg.output_channels) TG_CHECK_ARG(ch >= 0 && ch < (int)cfg.types.size(), "output channel out of range");
    TG_CHECK_ARG(cfg.expected_positions > 0, "expected positions must be positive");   // WindowOperator.java:120
}

// =====================================================================================================================
// LimitOperator (M/operator/LimitOperator.java:62-119): whole pages pass through while they fit, the crossing page is a region of its
// first `remaining` rows, finish() zeroes the remainder.  No kernel.
// =====================================================================================================================
class LimitOperator : public PageOperator {
public:
    LimitOperator(Context *ctx, int32_t id, const LimitConfig &cfg) : PageOperator(ctx, id), types_(cfg.types), remaining_(cfg.limit) {}

    bool needs_input() override { return remaining_ > 0 && !pending_; }           // :92-96
    void finish() override { remaining_ = 0; }                                    // :80-84
    bool is_finished() override { return remaining_ == 0 && !pending_; }          // :86-90

private:
    void ready() override { TG_CHECK_STATE(needs_input(), "Operator does not need input"); }   // :101

    void emit(DevicePage in) override   // :98-111
    {
        check_page_types(in, types_);
        own_borrowed_columns(ctx_, in);
        if (in.n <= remaining_) {
            remaining_ -= in.n;
        }
        else {
            for (DeviceColumn &c : in.cols) c = k::region_of(ctx_, c, 0, remaining_);
            in.n = remaining_;
            remaining_ = 0;
        }
        pending_ = wrap(std::move(in));
    }

    std::vector<int32_t> types_;
    int64_t remaining_;
};

static void validate(Context *, const LimitConfig &cfg)
{
    TG_CHECK_ARG(!cfg.types.empty(), "limit needs at least one source channel");
    for (int32_t t : cfg.types) TG_CHECK_ARG(valid_type(t), "unknown type");
    TG_CHECK_ARG(cfg.limit >= 0, "limit must be at least zero");   // :70
}

void Operator::add_input_owned(const DevicePage &page)
{
    std::vector<tgpu_block> blocks(page.cols.size());
    for (size_t i = 0; i < page.cols.size(); i++) {
        const DeviceColumn &c = page.cols[i];
        blocks[i] = tgpu_block{c.type, TGPU_FLAT, TGPU_DEVICE, (int32_t)c.n, c.values, c.nulls, c.offsets, nullptr, nullptr};
    }
    tgpu_page p{(int32_t)page.n, (int32_t)blocks.size(), blocks.data()};
    add_input(&p);
}

// =====================================================================================================================
// MergePages (M/operator/project/MergePages.java:86-190, MergePagesTransformation.process): the transformation the reference
// puts behind every PageProcessor, as an operator.  A page with at least min_row_count rows or min_page_size_in_bytes bytes
// passes through untouched (after whatever is buffered); smaller pages are appended to a buffer in HBM that is flushed when it
// reaches max_page_size_in_bytes (PageBuilder.isFull, S/PageBuilder.java:126-129) or at finish.  Sizes are the reference's
// accounting: (width + 1) bytes per fixed-width cell, length + 5 per VARCHAR cell (S/block/LongArrayBlock.java:69,
// VariableWidthBlock.java:121-124 and the matching BlockBuilder.addBytes calls).  In front of the GPU operators the thresholds
// are set to tens or hundreds of MB (DESIGN.md "Page granularity"); the reference's 1 MB cap on min_page_size_in_bytes
// (MergePages.java:58,107) is therefore not enforced.
// =====================================================================================================================
class MergePagesOperator : public Operator {
public:
    MergePagesOperator(Context *ctx, int32_t id, const MergePagesConfig &cfg)
        : Operator(ctx, id), types_(cfg.types), min_page_size_(cfg.min_page_size_in_bytes), max_page_size_(cfg.max_page_size_in_bytes), min_row_count_(cfg.min_row_count)
    {
    }

    bool needs_input() override { return !finishing_ && output_.empty(); }

    void add_input(const tgpu_page *page) override { merge(ingest_page(ctx_, page)); }
    void add_input_owned(const DevicePage &page) override { merge(DevicePage(page)); }   // shares the page's buffers

    void merge(DevicePage in)
    {
        TG_CHECK_STATE(needs_input(), "Operator does not need input");
        check_page_types(in, types_);
        std::vector<std::array<int32_t, 2>> ends;
        const int64_t size = in.n >= min_row_count_ ? 0 : java_size_in_bytes(in, ends);   // (only needed to classify a page with few rows)
        if (in.n >= min_row_count_ || size >= min_page_size_) {   // :145-157
            flush();
            output_.push_back(owned(std::move(in)));
            return;
        }
        if (in.n == 0) return;
        if (!buffer_) buffer_ = std::make_unique<PagesIndexGpu>(ctx_, types_);
        buffer_->add_page(in, &ends);   // :159 appendPage
        buffered_size_ += size;
        if (buffered_size_ >= max_page_size_ || buffer_->position_count() == 0x7fffffffLL) flush();   // :161-163
    }

    std::unique_ptr<OutputPage> get_output() override
    {
        if (output_.empty()) return nullptr;
        DevicePage p = std::move(output_.front());
        output_.pop_front();
        return wrap(std::move(p));
    }

    void finish() override
    {
        if (!finishing_) flush();   // :134-142
        finishing_ = true;
    }
    bool is_finished() override { return finishing_ && output_.empty(); }
    int64_t memory_bytes() override
    {
        int64_t s = buffer_ ? buffer_->estimated_size() : 0;
        for (auto &p : output_) s += p.size_in_bytes();
        return s;
    }

private:
    // Page.getSizeInBytes of flat blocks.  The byte range of a VARCHAR channel is known on the host for pages that came through the
    // host ingest; for device-resident input it comes back in one batched read (the only synchronisation of the per-page path)
    int64_t java_size_in_bytes(const DevicePage &p, std::vector<std::array<int32_t, 2>> &ends)
    {
        int64_t s = 0;
        ends.assign(p.cols.size(), {0, 0});
        std::vector<Context::Transfer> reads;
        for (size_t i = 0; i < p.cols.size(); i++) {
            const DeviceColumn &c = p.cols[i];
            if (c.type != TGPU_VARCHAR) s += (int64_t)(type_width(c.type) + 1) * p.n;
            else if (c.pool_exact) ends[i] = {c.pool_first, (int32_t)c.pool_bytes};
            else if (p.n > 0) {
                reads.push_back({&ends[i][0], c.offsets, 4});
                reads.push_back({&ends[i][1], c.offsets + p.n, 4});
            }
        }
        if (!reads.empty()) ctx_->download_batch(reads);
        for (size_t i = 0; i < p.cols.size(); i++)
            if (p.cols[i].type == TGPU_VARCHAR) s += ((int64_t)ends[i][1] - ends[i][0]) + 5 * p.n;
        return s;
    }

    // a page that passes through must outlive the call: device-resident input is borrowed (common.h), so it is copied once
    DevicePage owned(DevicePage &&p)
    {
        bool borrowed = false;
        for (auto &c : p.cols) borrowed = borrowed || (c.n > 0 && !c.values_buf);
        if (!borrowed) return std::move(p);
        PagesIndexGpu copy(ctx_, types_);
        copy.add_page(p);
        DevicePage out;
        out.n = p.n;
        for (size_t i = 0; i < types_.size(); i++) out.cols.push_back(copy.column((int)i));
        return out;
    }

    void flush()
    {
        if (!buffer_ || buffer_->position_count() == 0) return;
        DevicePage out;
        out.n = buffer_->position_count();
        for (size_t i = 0; i < types_.size(); i++) out.cols.push_back(buffer_->column((int)i));
        output_.push_back(std::move(out));
        buffer_.reset();   // the flushed columns keep the buffers alive
        buffered_size_ = 0;
    }

    std::vector<int32_t> types_;
    int64_t min_page_size_, max_page_size_, buffered_size_ = 0;
    int32_t min_row_count_;
    bool finishing_ = false;
    std::unique_ptr<PagesIndexGpu> buffer_;
    std::deque<DevicePage> output_;
};

static void validate(Context *, const MergePagesConfig &cfg)   // MergePages.java:102-106
{
    TG_CHECK_ARG(cfg.min_page_size_in_bytes >= 0, "minPageSizeInBytes must be greater or equal than zero");
    TG_CHECK_ARG(cfg.min_row_count >= 0, "minRowCount must be greater or equal than zero");
    TG_CHECK_ARG(cfg.max_page_size_in_bytes > 0, "maxPageSizeInBytes must be greater than zero");
    TG_CHECK_ARG(cfg.max_page_size_in_bytes >= cfg.min_page_size_in_bytes, "maxPageSizeInBytes must be greater or equal than minPageSizeInBytes");
    for (int32_t t : cfg.types) TG_CHECK_ARG(valid_type(t), "unknown channel type");
}

// =====================================================================================================================
// PartitionedOutputOperator (M/operator/PartitionedOutputOperator.java; PagePartitioner.partitionPage :406-426)
//   position -> every partition when (replicatesAnyRow and no row has been replicated yet) or the null channel is null there,
//   else -> partitionFunction.getPartition = (rawHash & 0x7fff...) % partitionCount (HashGenerator.java:24-35) of the
//   precomputed hash channel or of the partition channels' InterpretedHashGenerator hash.
// Rows reach each partition in input order.  The reference appends them to per-partition PageBuilders and flushes full ones;
// here every input page is flushed as it is partitioned (page boundaries are not part of the exchange contract).
// =====================================================================================================================
namespace {
__global__ void __launch_bounds__(256) replicate_flags_kernel(const uint8_t *null_channel_nulls, int64_t n, int replicate_first, uint8_t *out)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        out[i] = (uint8_t)(((null_channel_nulls && null_channel_nulls[i]) || (replicate_first && i == 0)) ? 1 : 0);
}
}  // namespace

class PartitionedOutputOperator : public Operator {
public:
    PartitionedOutputOperator(Context *ctx, int32_t id, const PartitionedOutputConfig &cfg)
        : Operator(ctx, id), types_(cfg.types), partition_channels_(cfg.partition_channels), hash_channel_(cfg.hash_channel), partition_count_(cfg.partition_count),
          null_channel_(cfg.null_channel), replicates_any_row_(cfg.replicates_any_row), local_function_(cfg.partition_function == TGPU_PARTITION_LOCAL)
    {
    }

    bool needs_input() override { return !finishing_; }   // :268-271 (the output buffer's back pressure is the shim's business)

    void add_input(const tgpu_page *page) override
    {
        TG_CHECK_STATE(!finishing_, "Operator is already finishing");
        DevicePage in = ingest_page(ctx_, page);
        check_page_types(in, types_);
        const int64_t n = in.n;
        if (n == 0) return;   // :274-277
        BufferPtr own_hashes;
        auto [keys, hashes] = key_inputs(in, partition_channels_, hash_channel_);
        if (hash_channel_ < 0) {
            own_hashes = ctx_->alloc((size_t)n * 8);
            k::hash_rows(ctx_, key_cols_of(keys), n, own_hashes->as<int64_t>());
            hashes = own_hashes->as<int64_t>();
        }
        BufferPtr ids = ctx_->alloc((size_t)n * 4), cnt = ctx_->alloc((size_t)partition_count_ * 8);
        k::partition_ids(ctx_, hashes, n, partition_count_, ids->as<int32_t>(), local_function_);
        // replicated rows of this page
        const uint8_t *null_flags = null_channel_ >= 0 ? in.cols[(size_t)null_channel_].nulls : nullptr;
        const bool replicate_first = replicates_any_row_ && !has_any_row_been_replicated_;
        BufferPtr replicate;
        if (null_flags || replicate_first) {
            replicate = ctx_->alloc((size_t)n);
            replicate_flags_kernel<<<grid_for(ctx_, n), 256, 0, ctx_->stream()>>>(null_flags, n, replicate_first ? 1 : 0, replicate->as<uint8_t>());
            check_launch("replicate_flags");
            has_any_row_been_replicated_ = true;   // :411-418 (row 0 if the flag was pending; null rows replicate regardless)
        }
        BufferPtr positions;
        int64_t pairs = 0;
        k::partition_pairs(ctx_, ids->as<int32_t>(), replicate ? replicate->as<uint8_t>() : nullptr, n, partition_count_, positions, pairs, cnt->as<int64_t>());
        std::vector<int64_t> counts((size_t)partition_count_);
        ctx_->download(counts.data(), cnt->ptr(), (size_t)partition_count_ * 8);
        DevicePage grouped;
        grouped.n = pairs;
        for (auto &col : in.cols) grouped.cols.push_back(k::gather_column(ctx_, col, positions->as<int32_t>(), pairs, false));
        int64_t at = 0;
        for (int32_t p = 0; p < partition_count_; p++) {
            const int64_t len = counts[(size_t)p];
            if (len > 0) {
                DevicePage part;
                part.n = len;
                for (auto &col : grouped.cols) part.cols.push_back(k::region_of(ctx_, col, at, len));   // views: the buffers are shared
                pending_.push_back({p, std::move(part)});
                pages_added_++;
                rows_added_ += len;
            }
            at += len;
        }
    }

    std::unique_ptr<OutputPage> get_output() override { return nullptr; }   // :303-306
    void finish() override { finishing_ = true; }                              // :255-259 flush(true): nothing is held back here
    bool is_finished() override { return finishing_; }

    int64_t memory_bytes() override
    {
        int64_t s = 0;
        for (auto &e : pending_) s += e.second.size_in_bytes();
        return s;
    }

    bool poll(int32_t *partition, std::unique_ptr<OutputPage> *out)
    {
        if (pending_.empty()) return false;
        *partition = pending_.front().first;
        *out = wrap(std::move(pending_.front().second));
        pending_.pop_front();
        return true;
    }
    // the largest number of pending pages any one partition has (a consumer that moves one page per partition and call checks BEFORE it polls)
    size_t max_pending_per_partition() const
    {
        std::vector<size_t> cnt((size_t)partition_count_, 0);
        size_t most = 0;
        for (auto &pp : pending_) most = std::max(most, ++cnt[(size_t)pp.first]);
        return most;
    }
    int32_t partition_count() const { return partition_count_; }
    int64_t rows_added_ = 0, pages_added_ = 0;   // PartitionedOutputInfo (:396-399)

private:
    std::vector<int32_t> types_, partition_channels_;
    int32_t hash_channel_, partition_count_, null_channel_;
    bool replicates_any_row_, local_function_, has_any_row_been_replicated_ = false, finishing_ = false;
    std::deque<std::pair<int32_t, DevicePage>> pending_;
};

static void validate(Context *, const PartitionedOutputConfig &cfg)
{
    const int nt = (int)cfg.types.size();
    TG_CHECK_ARG(cfg.partition_count > 0 && cfg.partition_count <= 1024, "partition count must be in 1..1024");
    TG_CHECK_ARG(cfg.partition_function == TGPU_PARTITION_HASH_MODULO || cfg.partition_function == TGPU_PARTITION_LOCAL, "unknown partition function");
    if (cfg.partition_function == TGPU_PARTITION_LOCAL)
        TG_CHECK_ARG((cfg.partition_count & (cfg.partition_count - 1)) == 0, "the local partition function needs a power-of-two partition count");
    TG_CHECK_ARG(cfg.null_channel < nt, "null channel out of range");
    if (cfg.hash_channel >= 0) TG_CHECK_ARG(cfg.hash_channel < nt && cfg.types[(size_t)cfg.hash_channel] == TGPU_BIGINT, "bad hash channel");
    else TG_CHECK_ARG(!cfg.partition_channels.empty(), "partitioning needs partition channels or a hash channel");
    for (int32_t ch : cfg.partition_channels) {
        // (a negative channel = a constant partitioning argument in the reference, :433-448)
        if (ch < 0) fail(TGPU_ERR_NOT_SUPPORTED, "constant partitioning arguments are not supported");
        TG_CHECK_ARG(ch < nt, "partition channel out of range");
    }
    TG_CHECK_ARG((int)cfg.partition_channels.size() <= kMaxKeyChannels, "at most 8 partition channels are supported");
}

bool partitioned_output_poll(Operator *op, int32_t *partition, std::unique_ptr<OutputPage> *out)
{
    auto *p = dynamic_cast<PartitionedOutputOperator *>(op);
    TG_CHECK_ARG(p != nullptr, "not a PartitionedOutputOperator");
    return p->poll(partition, out);
}

void partitioned_output_pending(Operator *op, size_t *max_per_partition, int32_t *partition_count)
{
    auto *p = dynamic_cast<PartitionedOutputOperator *>(op);
    TG_CHECK_ARG(p != nullptr, "not a PartitionedOutputOperator");
    *max_per_partition = p->max_pending_per_partition();
    *partition_count = p->partition_count();
}

void partitioned_output_info(Operator *op, int64_t *rows_added, int64_t *pages_added)
{
    auto *p = dynamic_cast<PartitionedOutputOperator *>(op);
    TG_CHECK_ARG(p != nullptr, "not a PartitionedOutputOperator");
    *rows_added = p->rows_added_;
    *pages_added = p->pages_added_;
}

// the plain factories (operators.h): instantiated here, where the operator classes are complete
template class SimpleOperatorFactory<FilterAndProjectConfig, FilterAndProjectOperator>;
template class SimpleOperatorFactory<ScanFilterAndProjectConfig, ScanFilterAndProjectOperator>;
template class SimpleOperatorFactory<HashAggregationConfig, HashAggregationOperator>;
template class SimpleOperatorFactory<StreamingAggregationConfig, StreamingAggregationOperator>;
template class SimpleOperatorFactory<TopNConfig, TopNOperator>;
template class SimpleOperatorFactory<OrderByConfig, OrderByOperator>;
template class SimpleOperatorFactory<MergeConfig, MergeOperator>;
template class SimpleOperatorFactory<DynamicFilterSourceConfig, DynamicFilterSourceOperator>;
template class SimpleOperatorFactory<HashSemiJoinConfig, HashSemiJoinOperator>;
template class SimpleOperatorFactory<MarkDistinctConfig, MarkDistinctOperator>;
template class SimpleOperatorFactory<DistinctLimitConfig, DistinctLimitOperator>;
template class SimpleOperatorFactory<RowNumberConfig, RowNumberOperator>;
template class SimpleOperatorFactory<LimitConfig, LimitOperator>;
template class SimpleOperatorFactory<TopNRankingConfig, TopNRankingOperator>;
template class SimpleOperatorFactory<WindowConfig, WindowOperator>;
template class SimpleOperatorFactory<MergePagesConfig, MergePagesOperator>;
template class SimpleOperatorFactory<PartitionedOutputConfig, PartitionedOutputOperator>;

}  // namespace tgpu
