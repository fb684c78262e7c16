"""Every environment switch the Python host layer reads is documented: the set of SRHIP_* / SRADSGAN_* keys that the .py files
under sradsgan_amd/ look up in os.environ equals the set of names in INTEGRATION.md's table "Host environment switches".  A switch
added later has to be documented there (or this fails), and a row cannot outlive its switch."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = r'(?:SRHIP|SRADSGAN)_\w+'


def _keys_read():
    read = re.compile(r'''os\.(?:environ(?:\.get|\.setdefault|\.pop)?\s*[\[(]|getenv\s*\()\s*['"](%s)['"]''' % KEY)
    keys = set()
    for path in glob.glob(os.path.join(ROOT, 'sradsgan_amd', '**', '*.py'), recursive=True):
        keys.update(read.findall(open(path).read()))
    return keys


def _keys_documented():
    text = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    section = text.split('### Host environment switches', 1)[1].split('\n#', 1)[0]
    return set(re.findall(r'^\| `(%s)` \|' % KEY, section, flags=re.M))


def test_every_host_switch_is_in_the_integration_table():
    read, documented = _keys_read(), _keys_documented()
    assert read and documented
    assert read == documented, 'undocumented: %s; documented but not read: %s' % (sorted(read - documented), sorted(documented - read))
