// The drop-in's host record of its members (usearch_amd/csrc/members.hpp: pure host logic) on its own, under the sanitizers: a fixed
// seeded script over every operation of `members_t`, with the invariants of the header checked after each step against a shadow
// that is as plain as can be (a key and a row per slot, and the freed slots in the order they were freed).
//   members_test IMAGE [REMOVED_KEY …]   IMAGE: a serialized index whose slot i holds key 1000 + i, or a tombstone for the keys listed
// Compiled and run by tests/test_host_logic.py.
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <deque>
#include <random>
#include <set>

#include "../../usearch_amd/csrc/members.hpp"

using namespace usearch_amd;

#define CHECK(condition)                                                                       \
    do {                                                                                       \
        if (!(condition)) {                                                                    \
            std::printf("FAILED %s:%d after step %d: %s\n", __FILE__, __LINE__, step, #condition); \
            std::exit(1);                                                                      \
        }                                                                                      \
    } while (0)

static int step = 0;

struct shadow_t {
    std::vector<std::uint64_t> keys;
    std::vector<std::vector<std::uint8_t>> rows;
    std::deque<std::uint32_t> ring;     // freed and not retaken, oldest first
    std::set<std::uint32_t> recycled;   // retaken since the device last caught up
};

static void check(members_t& members, const shadow_t& shadow) {
    const std::size_t bpv = members.bytes_per_vector;
    CHECK(members.size() == shadow.keys.size());
    std::size_t present = 0;
    members.each_key([&](std::size_t slot, std::uint64_t key) {
        CHECK(key == shadow.keys[slot]);
        present += key != free_key_k;
        if (key != free_key_k) // rows stay where their keys are
            CHECK(std::memcmp(members.row((std::uint32_t)slot), shadow.rows[slot].data(), bpv) == 0);
    });
    CHECK(members.present() == present);
    const members_t::lookup_t& lookup = members.lookup(); // names exactly the slots that are not free
    CHECK(lookup.size() == present);
    std::set<std::uint32_t> named;
    for (const auto& entry : lookup)
        CHECK(entry.first != free_key_k && shadow.keys[entry.second] == entry.first && named.insert(entry.second).second);
    if (!members.staged)
        return;
    CHECK(members.vectors.size() == members.keys.size() * bpv);
    CHECK(members.free_slots.size() - members.free_head == shadow.ring.size()); // the tombstones not yet retaken, oldest first
    for (std::size_t i = 0; i < shadow.ring.size(); ++i)
        CHECK(members.free_slots[members.free_head + i] == shadow.ring[i] && shadow.keys[shadow.ring[i]] == free_key_k);
    CHECK(shadow.ring.size() == shadow.keys.size() - present);
    CHECK(members.has_free_slot() == !shadow.ring.empty());
    for (std::uint32_t slot : members.recycled)
        CHECK(slot < members.size() && shadow.recycled.count(slot));
    CHECK(members.has_stale() == !shadow.recycled.empty());
}

int main(int argc, char** argv) {
    if (argc < 2)
        return std::printf("usage: members_test IMAGE [REMOVED_KEY …]\n"), 2;
    std::set<std::uint64_t> removed_in_image;
    for (int i = 2; i < argc; ++i)
        removed_in_image.insert(std::strtoull(argv[i], nullptr, 10));
    const int fd = ::open(argv[1], O_RDONLY);
    struct stat st;
    if (fd < 0 || ::fstat(fd, &st) != 0)
        return std::printf("cannot read %s\n", argv[1]), 2;
    std::vector<std::uint8_t> file((std::size_t)st.st_size);
    if (::read(fd, file.data(), file.size()) != (ssize_t)file.size())
        return std::printf("cannot read %s\n", argv[1]), 2;

    std::mt19937_64 random(2024);
    members_t members;
    shadow_t shadow;
    std::uint64_t serial = 0;
    bool multi = false;

    const auto open_image = [&](int form) { // 0: a copy the record owns, 1: borrowed, 2: a mapping it releases
        image_bytes_t bytes = form == 0   ? copied_bytes(file.data(), file.size())
                              : form == 1 ? held_bytes(file.data(), file.size(), image_release_t::borrowed_k)
                                          : held_bytes(::mmap(nullptr, file.size(), PROT_READ, MAP_PRIVATE, fd, 0), file.size(), image_release_t::mapped_k);
        image_t parsed;
        CHECK((const void*)bytes.get() != MAP_FAILED && parsed.open(bytes.get(), file.size()) == nullptr);
        members.open_image(std::move(bytes), parsed);
        CHECK(members.has_image() && !members.staged && members.image_length() == file.size());
        CHECK(members.host_bytes() >= (form == 0 ? file.size() : 0) && members.bytes_per_vector == parsed.cols);
        shadow = shadow_t();
        for (std::uint64_t slot = 0; slot < parsed.size; ++slot) {
            shadow.keys.push_back(removed_in_image.count(1000 + slot) ? free_key_k : 1000 + slot);
            shadow.rows.emplace_back(parsed.vectors + slot * parsed.cols, parsed.vectors + (slot + 1) * parsed.cols);
        }
        CHECK(members.present() == parsed.count_present);
    };
    const auto stage = [&] {
        if (!members.staged) // the image's tombstones are listed, lowest slot first
            for (std::size_t slot = 0; slot < shadow.keys.size(); ++slot)
                if (shadow.keys[slot] == free_key_k)
                    shadow.ring.push_back((std::uint32_t)slot);
        members.stage();
        CHECK(members.staged && !members.has_image());
    };
    const auto add = [&](std::uint64_t key) {
        stage();
        if (!multi && members.lookup().count(key))
            return;
        std::uint8_t* row = members.take_slot(key);
        CHECK(row != nullptr);
        const std::size_t slot = (std::size_t)(row - members.vectors.data()) / members.bytes_per_vector;
        std::vector<std::uint8_t> bytes(members.bytes_per_vector);
        for (std::uint8_t& byte : bytes)
            byte = (std::uint8_t)(++serial * 37);
        std::memcpy(row, bytes.data(), bytes.size()); // the caller writes the row
        if (!shadow.ring.empty()) { // the oldest freed slot first
            CHECK(slot == shadow.ring.front());
            shadow.ring.pop_front();
            shadow.recycled.insert((std::uint32_t)slot);
        } else {
            CHECK(slot == shadow.keys.size());
            shadow.keys.push_back(free_key_k), shadow.rows.emplace_back();
        }
        shadow.keys[slot] = key, shadow.rows[slot] = bytes;
    };
    const auto remove = [&](std::uint64_t key) {
        if (!members.lookup().count(key))
            return;
        stage();
        std::size_t expected = 0;
        for (std::uint64_t k : shadow.keys)
            expected += k == key;
        const std::size_t removed = members.remove(key, [&](std::uint32_t slot) {
            CHECK(shadow.keys[slot] == key);
            shadow.keys[slot] = free_key_k;
            shadow.ring.push_back(slot);
        });
        CHECK(removed == expected && expected != 0);
    };
    const auto rename = [&](std::uint64_t from, std::uint64_t to) {
        if (!members.lookup().count(from) || (!multi && members.lookup().count(to)))
            return;
        stage();
        std::size_t expected = 0;
        for (std::uint64_t k : shadow.keys)
            expected += k == from;
        const std::size_t renamed = members.rename(from, to, [&](std::uint32_t slot) {
            CHECK(shadow.keys[slot] == from);
            shadow.keys[slot] = to;
        });
        CHECK(renamed == expected);
    };
    const auto device_catches_up = [&](std::size_t linked) { // what `builder_t::update` is handed
        const members_t::stale_t stale = members.stale(linked);
        CHECK(stale.keys.size() == stale.slots.size() && stale.rows.size() == stale.slots.size() * members.bytes_per_vector);
        std::set<std::uint32_t> expected;
        for (std::uint32_t slot : shadow.recycled)
            if (slot < linked && shadow.keys[slot] != free_key_k)
                expected.insert(slot);
        CHECK(std::set<std::uint32_t>(stale.slots.begin(), stale.slots.end()) == expected && stale.slots.size() == expected.size());
        for (std::size_t i = 0; i < stale.slots.size(); ++i) {
            CHECK(i == 0 || stale.slots[i - 1] < stale.slots[i]);
            CHECK(stale.keys[i] == shadow.keys[stale.slots[i]]);
            CHECK(std::memcmp(stale.rows.data() + i * members.bytes_per_vector, shadow.rows[stale.slots[i]].data(), members.bytes_per_vector) == 0);
        }
        members.settle_stale();
        shadow.recycled.clear();
    };
    const auto compact = [&] { // the map a device compaction reports: tombstones dropped, survivors in order
        stage();
        std::vector<std::uint32_t> slot_map(shadow.keys.size(), none_slot_k);
        shadow_t after;
        for (std::size_t slot = 0; slot < shadow.keys.size(); ++slot)
            if (shadow.keys[slot] != free_key_k) {
                slot_map[slot] = (std::uint32_t)after.keys.size();
                after.keys.push_back(shadow.keys[slot]), after.rows.push_back(shadow.rows[slot]);
            }
        members.compact(slot_map.data(), after.keys.size());
        shadow = after;
    };
    const auto clear = [&] {
        members.clear();
        shadow = shadow_t();
        CHECK(!members.staged && !members.has_image() && members.size() == 0);
    };

    for (int round = 0; round < 6; ++round) {
        multi = round % 2 == 1;
        if (round < 3) {
            open_image(round);
            check(members, shadow); // key, row and lookup straight from the image
        } else {
            members.bytes_per_vector = 16;
            members.reserve(64);
        }
        for (int i = 0; i < 400; ++i, ++step) {
            const std::uint64_t key = 1000 + random() % 80, other = 1000 + random() % 80;
            const unsigned draw = (unsigned)(random() % 100);
            if (draw < 45)
                add(key);
            else if (draw < 70)
                remove(key);
            else if (draw < 85)
                rename(key, other);
            else if (draw < 93)
                device_catches_up(members.staged ? random() % (members.size() + 1) : 0);
            else if (draw < 97)
                compact();
            else if (draw < 98 && round == 4)
                clear();
            check(members, shadow);
        }
        if (round == 1) { // an image that is let go before anything staged it takes its key table along
            open_image(1);
            check(members, shadow);
            members.drop_image();
            shadow = shadow_t();
            check(members, shadow);
        }
        clear();
        check(members, shadow);
    }
    ::close(fd);
    std::printf("PASSED %d steps\n", step);
    return 0;
}
