/**
 *  usearch_amd/csrc/members.hpp — the host's record of an index's members, as the drop-in C ABI keeps it (dropin.hip): what the
 *  reference keeps in `index_dense_gt` — a key and a vector per slot, for `get`, `contains`, `count`, `rename`, `remove` — plus the
 *  ring of slots a removal freed (`free_keys_`, index_dense.hpp:507, 1479-1511). Pure host logic: no HIP, no locks, no device state;
 *  when `version` moves and when the device copy is dropped is the caller's business (tests/cpp/members_test.cpp runs it alone).
 *
 *  The record has one of two forms:
 *    an image   the serialized bytes as loaded or viewed; keys are read off the node tapes, rows out of its matrix;
 *    staged     `keys` and `vectors` per slot, from the first change on (`stage()` moves an image over and lets go of it).
 *  What holds between calls:
 *    - `lookup()` names exactly the slots whose key is not `free_key_k`;
 *    - staged: `free_slots[free_head …]` are exactly the tombstoned slots no add has retaken, oldest first; an image's tombstones
 *      are listed by `stage()`, lowest slot first (what `reindex_keys_` does after a load, index_dense.hpp:2162-2200);
 *    - `recycled` holds retaken slots whose device copy still shows the member that was removed: all below `size()`;
 *    - `vectors` holds `bytes_per_vector` bytes per slot of `keys`: a row stays where its key is.
 */
#pragma once
#include <sys/mman.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <memory>
#include <unordered_map>
#include <vector>

#include "common.hpp"
#include "image.hpp"

namespace usearch_amd {

/// The bytes of an image and how they are let go: a copy the index owns, a buffer the caller keeps alive, or a mapped file.
struct image_release_t {
    enum how_t { borrowed_k, owned_k, mapped_k } how = borrowed_k;
    std::size_t length = 0;
    void operator()(const std::uint8_t* bytes) const {
        if (how == owned_k)
            delete[] bytes;
        else if (how == mapped_k)
            ::munmap(const_cast<std::uint8_t*>(bytes), length);
    }
};
using image_bytes_t = std::unique_ptr<const std::uint8_t[], image_release_t>;

inline image_bytes_t held_bytes(const void* bytes, std::size_t length, image_release_t::how_t how) {
    return image_bytes_t(static_cast<const std::uint8_t*>(bytes), image_release_t{how, length});
}
inline image_bytes_t copied_bytes(const void* bytes, std::size_t length) {
    std::uint8_t* copy = new std::uint8_t[length];
    if (length)
        std::memcpy(copy, bytes, length);
    return held_bytes(copy, length, image_release_t::owned_k);
}

struct members_t {
    using lookup_t = std::unordered_multimap<std::uint64_t, std::uint32_t>;
    image_bytes_t bytes; ///< the image, while the index is one (null otherwise)
    image_t image;       ///< its parsed header
    bool staged = false;
    std::size_t bytes_per_vector = 0; ///< of the index's scalar kind and dimensions: set with them
    std::vector<std::uint64_t> keys;
    std::vector<std::uint8_t> vectors; ///< storage scalar kind, `bytes_per_vector` per slot
    std::vector<std::uint32_t> free_slots;
    std::size_t free_head = 0;
    std::vector<std::uint32_t> recycled;

    bool has_image() const { return bytes != nullptr; }
    std::size_t image_length() const { return bytes.get_deleter().length; }
    /// Slots, tombstones included.
    std::size_t size() const { return staged ? keys.size() : has_image() ? (std::size_t)image.size : 0; }
    /// Members a search can find.
    std::size_t present() const {
        return staged ? keys.size() - (std::size_t)std::count(keys.begin(), keys.end(), free_key_k) : (std::size_t)image.count_present;
    }
    /// Host memory behind the record: the reserved staging arrays and an owned image.
    std::size_t host_bytes() const {
        return (bytes.get_deleter().how == image_release_t::owned_k ? image_length() : 0) + vectors.capacity() + keys.capacity() * 8;
    }

    /// Takes `parsed`, the header `image_t::open` read from `taken`, as the members; whatever was staged goes.
    void open_image(image_bytes_t&& taken, const image_t& parsed) {
        clear();
        bytes = std::move(taken), image = parsed;
        bytes_per_vector = (std::size_t)parsed.cols;
    }
    void drop_image() {
        if (!staged)
            lookup_valid_ = false; // it named the image's slots
        bytes = image_bytes_t();
        image = image_t{};
    }
    void clear() {
        drop_image();
        keys.clear(), vectors.clear();
        reset_ring();
        staged = false;
        lookup_.clear(), lookup_valid_ = false;
    }
    /// Room for `usearch_add` to put members without growing (an image is not where they go).
    void reserve(std::size_t capacity) {
        if (staged || !has_image())
            keys.reserve(capacity), vectors.reserve(capacity * bytes_per_vector);
    }

    /// `visit(slot, key)` for every slot in slot order, whichever form the index is in (an image's node tapes are variable-length:
    /// one sequential pass).
    template <typename visit_at> void each_key(visit_at&& visit) const {
        if (staged) {
            for (std::size_t slot = 0; slot < keys.size(); ++slot)
                visit(slot, keys[slot]);
            return;
        }
        std::size_t offset = 0;
        for (std::size_t slot = 0; slot < size(); ++slot) {
            visit(slot, image_t::load<std::uint64_t>(image.tapes + offset));
            offset += image.node_bytes(image.level(slot));
        }
    }
    const std::uint8_t* row(std::uint32_t slot) const {
        return staged ? vectors.data() + (std::size_t)slot * bytes_per_vector : image.vectors + (std::size_t)slot * image.cols;
    }
    /// key → slots, rebuilt lazily.
    const lookup_t& lookup() {
        if (!lookup_valid_) {
            lookup_.clear();
            lookup_.reserve(size());
            each_key([&](std::size_t slot, std::uint64_t key) {
                if (key != free_key_k)
                    lookup_.emplace(key, (std::uint32_t)slot);
            });
            lookup_valid_ = true;
        }
        return lookup_;
    }

    /// Moves keys and rows out of the image into the staging arrays and lists its tombstones: the index is about to change.
    void stage() {
        if (staged)
            return;
        if (has_image()) {
            keys.resize((std::size_t)image.size);
            each_key([&](std::size_t slot, std::uint64_t key) { keys[slot] = key; });
            vectors.assign(image.vectors, image.vectors + (std::size_t)image.size * image.cols);
        }
        reset_ring();
        for (std::size_t slot = 0; slot < keys.size(); ++slot)
            if (keys[slot] == free_key_k)
                free_slots.push_back((std::uint32_t)slot);
        staged = true;
        drop_image();
        lookup_valid_ = false;
    }

    bool has_free_slot() const { return staged && free_head < free_slots.size(); }
    /// A slot for a new member of a staged index: the oldest freed one first (`free_keys_.try_pop`, index_dense.hpp:1479-1511), noted
    /// as recycled, else a new one. → where the caller writes the row (it owns the casts), or null when 32-bit slots run out.
    std::uint8_t* take_slot(std::uint64_t key) {
        std::size_t slot = keys.size();
        if (has_free_slot()) {
            slot = free_slots[free_head++];
            keys[slot] = key;
            recycled.push_back((std::uint32_t)slot);
            if (free_head == free_slots.size())
                free_slots.clear(), free_head = 0;
        } else {
            if (slot + 1 >= none_slot_k)
                return nullptr;
            vectors.resize((slot + 1) * bytes_per_vector);
            keys.push_back(key);
        }
        if (lookup_valid_)
            lookup_.emplace(key, (std::uint32_t)slot);
        return vectors.data() + slot * bytes_per_vector;
    }
    /// Every slot of `key` becomes a tombstone and joins the ring; `each(slot)` per slot. → how many.
    template <typename each_at> std::size_t remove(std::uint64_t key, each_at&& each) {
        const auto range = lookup().equal_range(key);
        std::size_t removed = 0;
        for (auto it = range.first; it != range.second; ++it, ++removed) {
            keys[it->second] = free_key_k;
            free_slots.push_back(it->second);
            each(it->second);
        }
        lookup_.erase(key);
        return removed;
    }
    /// Every slot of `from` goes by `to`; `each(slot)` per slot. → how many.
    template <typename each_at> std::size_t rename(std::uint64_t from, std::uint64_t to, each_at&& each) {
        std::vector<std::uint32_t> slots;
        const auto range = lookup().equal_range(from);
        for (auto it = range.first; it != range.second; ++it)
            slots.push_back(it->second);
        lookup_.erase(from);
        for (std::uint32_t slot : slots) {
            keys[slot] = to;
            lookup_.emplace(to, slot);
            each(slot);
        }
        return slots.size();
    }
    /// The staging arrays after a compaction: slot → `slot_map[slot]` (≤ slot, so everything moves down in place; `none_slot_k` =
    /// dropped), `survivors` slots remain and none of them is free.
    void compact(const std::uint32_t* slot_map, std::size_t survivors) {
        for (std::size_t slot = 0; slot < keys.size(); ++slot) {
            const std::uint32_t to = slot_map[slot];
            if (to == none_slot_k || to == slot)
                continue;
            keys[to] = keys[slot];
            std::memmove(vectors.data() + (std::size_t)to * bytes_per_vector, vectors.data() + slot * bytes_per_vector, bytes_per_vector);
        }
        keys.resize(survivors);
        vectors.resize(survivors * bytes_per_vector);
        reset_ring();
        lookup_valid_ = false;
    }

    /// What a device copy of the first `linked` slots still holds stale: the retaken slots among them that have a member, with the
    /// keys and rows they have now (`builder_t::update` links them anew). `settle_stale()` once the device has them.
    struct stale_t {
        std::vector<std::uint32_t> slots;
        std::vector<std::uint64_t> keys;
        std::vector<std::uint8_t> rows;
    };
    bool has_stale() const { return !recycled.empty(); }
    void settle_stale() { recycled.clear(); }
    stale_t stale(std::size_t linked) {
        stale_t out;
        std::sort(recycled.begin(), recycled.end());
        recycled.erase(std::unique(recycled.begin(), recycled.end()), recycled.end());
        for (std::uint32_t slot : recycled)
            if (slot < linked && keys[slot] != free_key_k) {
                out.slots.push_back(slot);
                out.keys.push_back(keys[slot]);
                out.rows.insert(out.rows.end(), row(slot), row(slot) + bytes_per_vector);
            }
        return out;
    }

  private:
    lookup_t lookup_;
    bool lookup_valid_ = false;
    void reset_ring() { free_slots.clear(), free_head = 0, recycled.clear(); }
};

} // namespace usearch_amd
